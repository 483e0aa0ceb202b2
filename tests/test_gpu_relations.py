"""Distance / within relations between two patterns (kmpgpu_set_relations, kmpgpu_scan_relations, GpuMatcher.set_relations) on a
real MI355X.

The expectation is the host model of tests/match_model.py: the starts of every pattern, the hit matrix and the relation rows over
them.  counts come from the CPU oracle.  Every comparison is exact.

Run on a real MI355X:  python -m pytest tests/test_gpu_relations.py -m gpu
"""
import os
import random

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

from gpu_support import KERNELS, attach_slots, check_relations, check_rules, gm, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from match_model import I32_MAX, I32_MIN, U32_MAX  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, OPT_ACCUMULATE, OPT_FUSED, OPT_KERNEL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher)

ALPHABET = b"abcdAB"
EINVAL, ESTATE = -2, -3


def check_kernels(gm, oracle, payloads, pats, relations, windows=None, nocase=None, whole=False, kernels=KERNELS):
    st = MM.starts(payloads, pats, windows, nocase, whole)
    hits, rows = MM.hits(st), MM.relation_rows(st, pats, relations)
    counts = MM.oracle_counts(oracle, payloads, pats, nocase, whole)
    for name, kernel, fused in kernels:
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        check_relations(gm, rows, counts)
    gm.set_option(OPT_KERNEL, KERNEL_AUTO); gm.set_option(OPT_FUSED, 2)
    return hits, rows, counts


def place(L, items, fill=b"abcd", rng=None):
    """a payload of L bytes of filler with the (offset, bytes) items written into it (all of them fit)"""
    b = bytearray((rng.choice(fill) if rng else fill[i % len(fill)]) for i in range(L))
    for s, p in items:
        assert 0 <= s and s + len(p) <= L, (s, len(p), L)
        b[s:s + len(p)] = p
    return bytes(b)


def two_patterns(rng, m_a, m_b):
    """no letter of the filler, and the last byte of each nowhere else: a planted pattern starts where it was put and nowhere else"""
    return bytes(rng.choice(b"EFGH") for _ in range(m_a - 1)) + b"X", bytes(rng.choice(b"EFGH") for _ in range(m_b - 1)) + b"Y"


# ------------------------------------------------------------------------------------------------
# 1. bound edges: one A and one B with d = dmin - 1, dmin, dmax, dmax + 1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_a,m_b", [(3, 4), (1, 1), (99, 99), (1, 99), (99, 1), (16, 17)])
def test_bound_edges(gm, oracle, m_a, m_b):
    rng = random.Random(f"edges-{m_a}-{m_b}")
    A, B = two_patterns(rng, m_a, m_b)
    before = -(m_a + m_b)                             # d of a B that ends where A starts
    ranges = [(0, 0), (0, 20), (5, 5), (1, 70), (before - 20, before - 3), (before - 130, before), (before, 3),
              (None, 7), (-7 + before, None), (None, None), (None, before - 3), (64, None), (63, 64), (200, 1000)]
    relations = [(0, 1, lo, hi) for lo, hi in ranges]
    sa = 400
    payloads = []
    for lo, hi in ranges:
        for d in {x for x in (None if lo is None else lo - 1, lo, hi, None if hi is None else hi + 1) if x is not None}:
            sb = sa + m_a + d
            if sb < 0 or (sb < sa + m_a and sb + m_b > sa):
                continue                              # B would overlap A or start in front of the payload
            payloads.append(place(max(sa + m_a, sb + m_b) + rng.randrange(0, 40), [(sa, A), (sb, B)], rng=rng))
    payloads += [place(700, [(sa, A)]), place(700, [(sa, B)]), b""]
    try:
        reset(gm)
        gm.set_patterns([A, B])
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        assert gm.relations == relations
        hits, rows, _ = check_kernels(gm, oracle, payloads, [A, B], relations)
        # every relation both holds somewhere and fails on a payload that holds both patterns
        cand = hits[0] & hits[1]
        assert rows.any(axis=1).all()
        assert all((cand & ~rows[q]).any() for q, (lo, hi) in enumerate(ranges) if (lo, hi) != (None, None))
        assert (rows[ranges.index((None, None))] == cand).all()
        # the raw INT32 ends through the C-ABI are the same unbounded sides
        g = _lib.gpu_lib()
        arr = (_lib.Relation * 2)()
        arr[0].a, arr[0].b, arr[0].dmin, arr[0].dmax = 0, 1, I32_MIN, 7
        arr[1].a, arr[1].b, arr[1].dmin, arr[1].dmax = 0, 1, before - 7, I32_MAX
        assert g.kmpgpu_set_relations(gm._ctx, arr, 2) == 0
        gm.relations = [(0, 1, None, 7), (0, 1, before - 7, None)]
        res = gm.scan_relations(hits=True)
        assert (res["hits"] == rows[[ranges.index((None, 7)), ranges.index((-7 + before, None))]]).all()
    finally:
        reset(gm)


def test_overlapping_pair(gm, oracle):
    """B starts inside A: text PQRSTU holds PQRS at 0 and RSTU at 2, d = -2"""
    A, B = b"PQRS", b"RSTU"
    payloads = [place(L, [(s, b"PQRSTU")]) for L, s in ((6, 0), (70, 61), (200, 64), (1500, 1021))] + [place(90, [(3, A), (40, B)]), A + B, B + A]
    relations = [(0, 1, -2, -2), (0, 1, -1, 0), (0, 1, -3, -3), (0, 1, -5, -2), (0, 1, -2, 7), (0, 1, -1, None), (0, 1, None, -3),
                 (1, 0, -6, -6), (1, 0, -5, 0), (1, 0, None, None), (0, 1, 0, 0), (1, 0, 0, 0)]
    try:
        reset(gm)
        gm.set_patterns([A, B])
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        _, rows, _ = check_kernels(gm, oracle, payloads, [A, B], relations)
        assert rows[0, :4].all() and not rows[1, :4].any() and not rows[2, :4].any() and rows[7, :4].all()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. step edges of the sweep
# ------------------------------------------------------------------------------------------------
def test_sweep_step_edges(gm, oracle):
    rng = random.Random("steps")
    A, B = b"EFX", b"GHGY"
    m_a, m_b = len(A), len(B)
    payloads, relations = [], []
    for L in (0, 1, m_a + m_b - 1, m_a + m_b, 63, 64, 65, 127, 128, 129, 1024, 2200):
        if L < m_a + m_b:
            payloads.append(place(L, [(0, A)] if L >= m_a else []))
            continue
        d = L - m_b - m_a                             # A at the payload's start, B at its end
        payloads.append(place(L, [(0, A), (L - m_b, B)], rng=rng))
        payloads.append(place(L, [(L - m_a, A), (0, B)], rng=rng))             # and the other way round: d = -L
        relations += [(0, 1, d, d), (0, 1, d + 1, d + 70), (0, 1, max(d - 70, 0), d - 1) if d else (0, 1, 1, 1), (0, 1, -L, -L), (0, 1, min(1 - L, -m_a - m_b), -m_a - m_b)]
    # A ends a 64-offset step and B starts the next; A anywhere around the step's edge, B directly behind it or one byte on
    for s in (0, 1, 59, 60, 61, 62, 63, 64, 65, 124, 125, 126, 127, 128):
        payloads.append(place(s + m_a + m_b + 70, [(s, A), (s + m_a, B)], rng=rng))
        payloads.append(place(s + m_a + m_b + 70, [(s, A), (s + m_a + 1, B)], rng=rng))
        payloads.append(place(s + 300, [(s, A), (s + m_a + 64, B), (s + 200, B)], rng=rng))
    relations += [(0, 1, 0, 0), (0, 1, 1, 1), (0, 1, 0, 1), (0, 1, -3, 0), (0, 1, None, 0), (0, 1, 0, None), (0, 1, 64, 64), (0, 1, 63, 63),
                  (0, 1, 65, 200), (0, 1, 2, 63), (0, 1, 61, 61), (0, 1, 197 - m_a, 197 - m_a)]
    relations = sorted(set(relations), key=lambda r: (r[2] is None, r[2], r[3] is None, r[3]))
    try:
        reset(gm)
        gm.set_patterns([A, B])
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        _, rows, _ = check_kernels(gm, oracle, payloads, [A, B], relations)
        assert rows.any(axis=1).sum() >= 40                                     # (46 of the 54: the ones cut to lie beside a payload's d hold nowhere)
    finally:
        reset(gm)


def test_long_payload(gm, oracle):
    """66 000 bytes: A near the start, B near the end -- the carry of the last A over a thousand steps, offsets beyond 16 bits"""
    A, B = b"EFX", b"GHY"
    L, sa, sb = 66_000, 5, 65_990
    d = sb - (sa + len(A))
    payloads = [place(L, [(sa, A), (sb, B)]), place(300, [(sa, A), (200, B)]), b"", place(L, [(sa, A), (sb - 1, B)])]
    relations = [(0, 1, 0, d), (0, 1, 0, d - 1), (0, 1, d, None), (0, 1, d + 1, None), (0, 1, None, None), (0, 1, d, d),
                 (1, 0, -d - 6, -d - 6), (1, 0, -d - 5, 0), (1, 0, None, -d - 6), (0, 1, 65_536, 65_990), (0, 1, 0, 65_535)]
    try:
        reset(gm)
        gm.set_patterns([A, B])
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        _, rows, _ = check_kernels(gm, oracle, payloads, [A, B], relations)
        assert rows[0, 0] and not rows[1, 0] and rows[2, 0] and not rows[3, 0] and rows[1, 3] and rows[6, 0] and not rows[7, 0]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 3. several occurrences of A; a == b
# ------------------------------------------------------------------------------------------------
def test_several_occurrences(gm, oracle):
    A, B, C4 = b"EFX", b"GHY", b"EGGZ"
    payloads = [
        place(120, [(10, A), (40, A), (45, B)]),             # d = 32 and 2
        place(120, [(20, B), (30, A), (60, A)]),             # d = -13 and -43
        place(1500, [(10, A), (700, A), (705, B), (1400, A)]),
        place(120, [(10, C4), (50, C4)]),                    # d = 36, -44, and -4 with itself
        place(120, [(10, C4)]),
        place(300, [(s, A) for s in range(0, 280, 7)] + [(290, B)]),
        place(300, [(0, B)] + [(s, A) for s in range(10, 280, 7)]),
    ]
    relations = [(0, 1, 10, 40), (0, 1, 3, 31), (0, 1, 2, 2), (0, 1, 33, None),          # the nearest A is too near, an earlier one is in range
                 (0, 1, -45, -40), (0, 1, -12, -1), (0, 1, -42, -14), (0, 1, None, -44),  # the only A in range lies behind a nearer one
                 (2, 2, 36, 36), (2, 2, 1, 35), (2, 2, -4, -4), (2, 2, -3, None), (2, 2, None, -5), (2, 2, -44, -44), (2, 2, -43, -5), (2, 2, None, None),
                 (0, 0, -3, -3), (0, 0, 4, 4), (0, 0, 5, 5), (1, 1, 0, 0), (0, 1, 8, 8), (0, 1, 9, 9), (0, 1, -300, -284), (0, 1, 282, 290)]
    pats = [A, B, C4]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        _, rows, _ = check_kernels(gm, oracle, payloads, pats, relations)
        assert rows[0, 0] and not rows[1, 0] and rows[4, 1] and not rows[5, 1] and not rows[6, 1]
        assert rows[8, 3] and not rows[8, 4] and not rows[9, 3] and rows[10, 3] and rows[10, 4] and not rows[11, 4] and not rows[12, 4]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 4. the text's end
# ------------------------------------------------------------------------------------------------
def test_text_end(gm, oracle):
    rng = random.Random("end")
    A, B = b"EFX", b"GHY"
    payloads = []
    for k in range(70):
        L = rng.randrange(40, 1300)
        sa = rng.randrange(0, L - 30)
        sb = rng.randrange(sa + 3, L - 3)
        b = bytearray(place(L, [(sa, A), (sb, B)], rng=rng))
        z = [None, rng.randrange(sa + 3, sb + 1), rng.randrange(0, sa + 3), sb + 1, sb + 2, sb + 3 if sb + 3 < L else None][k % 6]
        if z is not None:
            b[z] = 0                                  # between the two; in front of both or inside A; inside B; directly behind B
        payloads.append(bytes(b))
    # a B that ends exactly at the payload's end, and one whose last byte lies in the slot's padding
    payloads += [place(50, [(4, A), (47, B)]), place(49, [(4, A)]) [:47] + B[:2], place(64, [(4, A), (61, B)]), place(63, [(4, A)])[:61] + B[:2]]
    slots = []
    for t in payloads:
        pad = (-len(t)) % 16 or (16 if not t else 0)
        slots.append(t + (b"Y" + B + A + b"Y" * 16)[:pad])         # the padding would complete the cut B
    relations = [(0, 1, 0, None), (0, 1, None, None), (1, 0, None, None), (0, 1, 0, 200), (0, 1, 40, 44), (0, 1, 54, 54)]
    try:
        reset(gm)
        gm.set_patterns([A, B])
        for attach in (False, True):
            keep = attach_slots(gm, payloads, slots) if attach else gm.load_arena(K.HostArena.from_payloads(payloads))
            gm.set_relations(relations)
            seen = {}
            for whole in (0, 1, 0):                   # switched between two calls with nothing reloaded
                gm.set_option(OPT_WHOLE_PAYLOAD, whole)
                seen[whole] = check_kernels(gm, oracle, payloads, [A, B], relations, whole=bool(whole))[1]
            assert (seen[1] | seen[0] == seen[1]).all() and seen[1].sum() > seen[0].sum() > 0
            n = len(payloads)
            assert seen[0][0, n - 4] and not seen[0][0, n - 3] and seen[0][0, n - 2] and not seen[1][0, n - 1]
            del keep
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. nocase: one pattern read from the arena, the other from its folded copy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nocase", [(False, True), (True, False), (True, True)], ids=["b", "a", "both"])
def test_nocase(gm, oracle, nocase):
    rng = random.Random(f"nocase-{nocase}")
    A, B = b"aBcA", b"bAd"
    payloads = []
    for _ in range(200):
        L = rng.randrange(0, 500)
        b = bytearray(rng.choice(b"abcdABCD") for _ in range(L))
        for _ in range(L // 60):
            p = rng.choice([A, B, A.lower(), B.upper(), A.swapcase()])
            s = rng.randrange(0, L - len(p) + 1)
            b[s:s + len(p)] = p
        payloads.append(bytes(b))
    pats = [A, B, b"-+-"]                              # (the third: a nocase pattern without a letter stays with the arena)
    flags = list(nocase) + [True]
    relations = [(0, 1, 0, 30), (1, 0, 0, 30), (0, 1, -20, -1), (0, 1, None, None), (0, 0, 1, 100), (1, 1, -3, -3), (0, 1, 100, None), (2, 0, None, None)]
    try:
        reset(gm)
        gm.set_patterns(pats, nocase=flags)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        hits, rows, _ = check_kernels(gm, oracle, payloads, pats, relations, nocase=flags)
        sens = MM.relation_rows(MM.starts(payloads, pats), pats, relations)
        assert rows[:7].any(axis=1).all() and (rows != sens).any()      # folding found pairs that the bytes as written do not hold
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. windows decide what a match is, and are pass state
# ------------------------------------------------------------------------------------------------
def test_windows(gm, oracle):
    A, B = b"EFX", b"GHY"
    payloads = [place(400, [(10, A), (100, A), (110, B)]),          # d = 97 and 7
                place(400, [(10, A), (110, B), (300, B)]),          # d = 97 and 287
                place(400, [(120, A), (110, B), (5, B)]),
                place(90, [(10, A), (20, B)])]
    relations = [(0, 1, 0, 10), (0, 1, 90, 100), (0, 1, 200, None), (0, 1, None, -1), (0, 1, None, None)]
    try:
        reset(gm)
        gm.set_patterns([A, B])
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        gm.set_rules([([0, 1, gm.rel(0)], []), ([0], [gm.rel(1)])])
        base = check_kernels(gm, oracle, payloads, [A, B], relations)[1]
        assert base[0, 0] and base[2, 1]
        for windows in ([(0, 50), (0, None)],                       # removes the only in-range A of relation 0 in payload 0
                        [(0, None), (0, 200)],                      # ... the only in-range B of relation 2 in payload 1
                        [(100, 100), (110, 110)], [(11, 99), (0, None)], [(0, None), (6, 19)]):
            gm.set_windows(windows)
            hits, rows, counts = check_kernels(gm, oracle, payloads, [A, B], relations, windows=windows)
            assert (rows != base).any()
            check_rules(gm, np.concatenate([hits, rows]), gm.rules, counts)            # the rules, set before the windows, stay valid
            gm.set_windows(None)                                     # cleared between two passes, nothing re-set
            assert (check_kernels(gm, oracle, payloads, [A, B], relations)[1] == base).all()
        gm.set_windows([(0, 50), (0, None)])
        assert not gm.scan_relations(hits=True)["hits"][0, 0]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 7. column and row edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pkts", [1, 63, 64, 65, 127, 128, 129, 8193])
def test_column_edges(gm, oracle, n_pkts):
    rng = random.Random(f"cols-{n_pkts}")
    A, B = b"EFX", b"GHY"
    payloads = []
    for k in range(n_pkts):
        r = k % 7 if k < n_pkts - 1 else 0              # candidates in the last payload
        d = [4, 30, 4, 4, 30, 4, 4][r]
        payloads.append(place(20 + d + (k % 50), [(2, A), (5 + d, B)]) if r in (0, 1, 4) else place(10 + k % 30, [(2, A)] if r == 2 else []))
    relations = [(0, 1, 0, 10), (0, 1, 11, 40), (1, 0, None, None), (0, 1, 5, 29)]
    try:
        reset(gm)
        gm.set_patterns([A, B])
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        hits, rows, counts = check_kernels(gm, oracle, payloads, [A, B], relations, kernels=KERNELS if n_pkts < 8000 else KERNELS[:1])
        assert rows[0, n_pkts - 1] and not rows[3].any()
        # the words as the C-ABI writes them: bits at n_pkts and above are 0
        W = (n_pkts + 63) // 64
        rc, any_w, hit_w = np.full(4, 7, np.uint64), np.full(W, U32_MAX, np.uint64), np.full((4, W), U32_MAX, np.uint64)
        assert _lib.gpu_lib().kmpgpu_scan_relations(gm._ctx, rc.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data, None, None) == 0
        bits = np.unpackbits(hit_w.view(np.uint8), axis=1, bitorder="little")
        assert (bits[:, :n_pkts].astype(bool) == rows).all() and not bits[:, n_pkts:].any()
        abits = np.unpackbits(any_w.view(np.uint8), bitorder="little")
        assert (abits[:n_pkts].astype(bool) == rows.any(axis=0)).all() and not abits[n_pkts:].any()
        assert rc.tolist() == rows.sum(axis=1).tolist()
    finally:
        reset(gm)


@pytest.mark.parametrize("n_rel", [1, 255, 256, 257, 5000])
def test_row_edges(gm, oracle, n_rel):
    rng = random.Random(f"rows-{n_rel}")
    pats = [b"EFX", b"GHY", b"ab", b"c"]
    payloads = []
    for k in range(100):
        L = rng.randrange(0, 120)
        b = bytearray(rng.choice(b"abcd") for _ in range(L))
        for p in pats[:2]:
            if L >= 10 and rng.random() < 0.7:
                s = rng.randrange(0, L - 3)
                b[s:s + 3] = p
        payloads.append(bytes(b))
    kinds = [(0, 1, 0, 20), (0, 1, 0, 20), (1, 0, 0, 20), (2, 3, 0, 0), (3, 2, -1, 4), (2, 2, 2, 9), (0, 2, None, -3), (3, 1, 5, None)]
    relations = [kinds[q % len(kinds)] if q % 3 else (rng.randrange(4), rng.randrange(4), -rng.randrange(0, 9), rng.randrange(0, 30)) for q in range(n_rel)]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        _, rows, _ = check_kernels(gm, oracle, payloads, pats, relations, kernels=KERNELS[:1])
        assert rows.any() and not rows.all()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 8. random differential
# ------------------------------------------------------------------------------------------------
def _random_case(seed):
    rng = random.Random(f"diff-{seed}")
    pats = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (1, 2, 2, 3, 4, 5)]
    relations = []
    for _ in range(40):
        lo = rng.randrange(-40, 40)
        relations.append((rng.randrange(6), rng.randrange(6), None if rng.random() < 0.1 else lo, None if rng.random() < 0.1 else lo + rng.randrange(0, 30)))
    return rng, pats, relations


def _random_payloads(rng, kind, n=300):
    payloads = []
    for _ in range(n):
        L = 333 if kind == "uniform" else 0 if (kind == "empty" and rng.random() < 0.5) else rng.randrange(0, 401)
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        if L and rng.random() < 0.3:
            b[rng.randrange(L)] = 0
        payloads.append(bytes(b))
    return payloads


@pytest.mark.parametrize("kind", ["uniform", "mixed", "empty", "dirty", "in_place"])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_differential(gm, oracle, seed, kind):
    rng, pats, relations = _random_case(seed)
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
        gm.set_relations(relations)
        for whole in (0, 1):
            gm.set_option(OPT_WHOLE_PAYLOAD, whole)
            hits, rows, _ = check_kernels(gm, oracle, payloads, pats, relations, whole=bool(whole))
            cand = np.array([hits[a] & hits[b] for a, b, _, _ in relations])
            assert rows.any() and (cand & ~rows).any()
    finally:
        reset(gm)
        del keep


# ------------------------------------------------------------------------------------------------
# 9. rules over relations
# ------------------------------------------------------------------------------------------------
def test_rules_over_relations(gm, oracle):
    rng, pats, relations = _random_case(7)
    payloads = _random_payloads(rng, "empty")
    windows = [(0, None), (3, 200), (0, None), (0, 100), (0, None), (1, None)]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        pattern_rules = [([0, 3], [4]), ([], [5])]
        gm.set_rules(pattern_rules)
        before = (gm.scan_packets(hits=True), gm.scan_rules(hits=True))
        gm.set_relations(relations)
        assert gm.rules == []
        R = gm.rel
        # a relation that holds in some of the payloads that hold both of its patterns: as a term it narrows "a and b"
        st0 = MM.starts(payloads, pats)
        hits0, rows0 = MM.hits(st0), MM.relation_rows(st0, pats, relations)
        qn = next(q for q, (a, b, _, _) in enumerate(relations) if rows0[q].any() and (hits0[a] & hits0[b] & ~rows0[q]).any())
        a0, b0 = relations[qn][:2]
        rules = [([a0, b0, R(qn)], []), ([a0], [R(qn)]), ([], [R(1)]), ([R(2), R(3)], []), ([R(4)], [R(5), 0]), ([R(6), R(7), R(8), R(9), 1, 2], [R(10)]), ([R(39)], []),
                 ([], [R(11), R(12)])]
        gm.set_rules(rules)
        for w in (None, windows):
            gm.set_windows(w)
            hits, rows, counts = check_kernels(gm, oracle, payloads, pats, relations, windows=w)
            for _, kernel, fused in KERNELS:
                gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
                check_rules(gm, np.concatenate([hits, rows]), rules, counts)
            gm.set_option(OPT_KERNEL, KERNEL_AUTO); gm.set_option(OPT_FUSED, 2)      # (as `before` was taken: the launches are compared below)
            want = MM.rule_rows(np.concatenate([hits, rows]), rules)
            empty = np.array([len(t) == 0 for t in payloads])
            assert want[2][empty].all() and empty.any()                 # all-negated: empty payloads match
            if w is None:
                assert (want[0] != MM.rule_rows(np.concatenate([hits, rows]), [([a0, b0], [])])[0]).any() and want[0].any() and want[1].any()
        gm.set_windows(None)
        # pattern-level calls return what they returned before there were relations
        gm.scan_relations()
        pk = gm.scan_packets(hits=True)
        gm.set_rules(pattern_rules)
        ru = gm.scan_rules(hits=True)
        for got, was in ((pk, before[0]), (ru, before[1])):
            for key in was:
                if key != "timing":
                    assert np.array_equal(got[key], was[key]), key
        gm.set_relations(None)
        assert gm.relations == [] and gm.rules == []
        gm.set_rules(pattern_rules)
        ru = gm.scan_rules(hits=True)
        assert all(np.array_equal(ru[key], before[1][key]) for key in before[1] if key != "timing")
        assert ru["timing"].launches == before[1]["timing"].launches
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 10. state and errors
# ------------------------------------------------------------------------------------------------
def test_state_and_errors(gm, oracle):
    rng, pats, relations = _random_case(11)
    relations = relations[:5]
    payloads = _random_payloads(rng, "mixed", n=150)
    g = _lib.gpu_lib()

    def call(ctx, rels):
        arr = (_lib.Relation * max(len(rels), 1))()
        for r, (a, b, lo, hi) in zip(arr, rels):
            r.a, r.b, r.dmin, r.dmax = a, b, lo, hi
        return g.kmpgpu_set_relations(ctx, arr, len(rels))

    try:
        reset(gm)
        with GpuMatcher(0) as fresh:
            assert call(fresh._ctx, [(0, 0, 0, 0)]) == ESTATE                       # no patterns set
            assert g.kmpgpu_set_relations(fresh._ctx, None, 0) == ESTATE
            assert g.kmpgpu_scan_relations(fresh._ctx, None, None, None, None, None) == ESTATE
            fresh.set_patterns(pats)
            fresh.load_arena(K.HostArena.from_payloads(payloads))
            assert g.kmpgpu_scan_relations(fresh._ctx, None, None, None, None, None) == ESTATE      # no relations set
            assert b"kmpgpu_scan_relations" in g.kmpgpu_last_error()
            with pytest.raises(Exception):
                fresh.rel(0)
        n = len(pats)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        rules = [([0, gm.rel(0)], []), ([], [gm.rel(4)])]
        gm.set_rules(rules)
        st = MM.starts(payloads, pats)
        hits, rows = MM.hits(st), MM.relation_rows(st, pats, relations)
        counts = MM.oracle_counts(oracle, payloads, pats)
        # every refused call leaves the relations and the rules set before in force
        for bad in ([(n, 0, 0, 0)], [(0, n, 0, 0)], [(0, 1, 0, 5), (0, U32_MAX, 0, 5)], [(0, 1, 5, 4)], [(0, 1, I32_MAX, I32_MIN)], [(0, 1, 1, 0), (0, 1, 0, 0)]):
            assert call(gm._ctx, bad) == EINVAL, bad
            assert b"kmpgpu_set_relations" in g.kmpgpu_last_error()
            check_relations(gm, rows, counts)
            check_rules(gm, np.concatenate([hits, rows]), rules, counts)
        assert g.kmpgpu_set_relations(gm._ctx, None, 3) == EINVAL
        # too many rows: n_pat + n_rel has to stay below 2^31 (the bound is checked before rel[] is read: one element is enough)
        one = (_lib.Relation * 1)()
        one[0].a, one[0].b, one[0].dmin, one[0].dmax = 0, 1, 0, 5
        for n_rel in ((1 << 31) - n, (1 << 31) - n + 1, (1 << 32) - n, U32_MAX):
            assert g.kmpgpu_set_relations(gm._ctx, one, n_rel) == EINVAL, n_rel
            assert b"kmpgpu_set_relations" in g.kmpgpu_last_error()
            check_relations(gm, rows, counts)
            check_rules(gm, np.concatenate([hits, rows]), rules, counts)
        with pytest.raises(Exception):
            gm.set_relations([(0, n, 0, 0)])
        assert gm.relations == relations and gm.rules == rules
        check_rules(gm, np.concatenate([hits, rows]), rules, counts)
        # the bound of a rule's term is n_pat + n_rel
        u32p = _lib.GPU_API["kmpgpu_set_rules"][1][1]
        off = np.array([0, 1], dtype=np.uint32)
        for term, rc in ((n + len(relations), EINVAL), ((n + len(relations)) | _lib.RULE_NOT, EINVAL), (n + len(relations) - 1, 0)):
            t = np.array([term], dtype=np.uint32)
            assert g.kmpgpu_set_rules(gm._ctx, off.ctypes.data_as(u32p), t.ctypes.data_as(u32p), 1) == rc, term
        gm.rules = [([n + len(relations) - 1], [])]
        check_rules(gm, np.concatenate([hits, rows]), gm.rules, counts)
        # a successful kmpgpu_set_relations drops the rules: the same relations again, and a clear
        for rels in (relations, []):
            gm.set_rules(rules if rels else [([0], [])])
            gm.set_relations(rels)
            assert gm.rules == []
            assert g.kmpgpu_scan_rules(gm._ctx, None, None, None, None, None) == ESTATE
        assert g.kmpgpu_scan_relations(gm._ctx, None, None, None, None, None) == ESTATE
        t = np.array([n], dtype=np.uint32)
        assert g.kmpgpu_set_rules(gm._ctx, off.ctypes.data_as(u32p), t.ctypes.data_as(u32p), 1) == EINVAL      # no relations: the bound is n_pat again
        # launches: the relation kernel is one launch behind the scan launches, and a profile records it
        gm.set_relations(relations)
        gm.profile_begin(64)
        pk = gm.scan_packets()
        n_pk = len(gm.profile_end(64))
        gm.profile_begin(64)
        rl = gm.scan_relations()
        n_rl = len(gm.profile_end(64))
        assert n_rl == n_pk + 1 and rl["timing"].launches == pk["timing"].launches == n_pk + 1
        gm.set_rules([([0], [])])
        gm.profile_begin(64)
        ru = gm.scan_rules()
        assert len(gm.profile_end(64)) == n_pk + 2 and ru["timing"].launches == n_pk + 2
        # the general kernel does not mark: refused as kmpgpu_scan_packets refuses it
        gm.set_option(OPT_KERNEL, 1)
        assert g.kmpgpu_scan_relations(gm._ctx, None, None, None, None, None) == EINVAL
        gm.set_option(OPT_KERNEL, KERNEL_AUTO)
        # the context's counters stay untouched
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        gm.scan_enqueue()
        check_relations(gm, rows, counts)
        assert gm.counts_read().tolist() == counts
        gm.set_option(OPT_ACCUMULATE, 0)
        # n_pkts == 0: zeros, nothing launched
        gm.load_arena(np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        res = gm.scan_relations(hits=True)
        assert res["rel_pkt_counts"].tolist() == [0] * len(relations) and res["counts"].tolist() == [0] * n
        assert res["hits"].shape == (len(relations), 0) and res["timing"].launches == 0
        # set_patterns drops the relations
        gm.load_arena(K.HostArena.from_payloads(payloads))
        check_relations(gm, rows, counts)
        gm.set_patterns(pats)
        assert gm.relations == [] and gm.rules == []
        assert g.kmpgpu_scan_relations(gm._ctx, None, None, None, None, None) == ESTATE
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 11. the fixture capture, loaded both ways
# ------------------------------------------------------------------------------------------------
def _fixture_relations(payloads, tokens):
    """three relations over tokens that co-occur in udp_1000.pcap, picked with the model: the pairs with the most candidates, bounded so
    that the first one holds in some of its candidates and not in others"""
    st = MM.starts(payloads, tokens)
    hits = MM.hits(st)
    both = (hits[:, None, :] & hits[None, :, :]).sum(axis=2)
    np.fill_diagonal(both, 0)
    pairs = [divmod(int(i), len(tokens)) for i in np.argsort(-both, axis=None)[:40]]
    for a, b in pairs:
        ds = sorted({min((y - (x + len(tokens[a])) for x in row[a] for y in row[b]), key=abs) for row in st if row[a] and row[b]})
        if len(ds) >= 3:
            mid = ds[len(ds) // 2]
            rel0 = (a, b, min(mid, 0), max(mid, 0))
            rows = MM.relation_rows(st, tokens, [rel0])
            if 0 < rows[0].sum() < both[a, b]:
                others = [p for p in pairs if p != (a, b) and set(p) != {a, b}][:2]
                return [rel0, (others[0][0], others[0][1], 0, 64), (others[1][0], others[1][1], None, -1)]
    raise AssertionError("no pair of tokens with hits and candidate misses")


@pytest.fixture(scope="module")
def capture(tokens):
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(arena.payload(k)) for k in range(arena.n_pkts)]
    relations = _fixture_relations(payloads, tokens)
    st = MM.starts(payloads, tokens)
    hits, rows = MM.hits(st), MM.relation_rows(st, tokens, relations)
    return arena, payloads, relations, hits, rows


def test_fixture_capture(gm, oracle, tokens, fixture_counts, capture):
    arena, payloads, relations, hits, rows = capture
    counts = fixture_counts["fixtures"]["udp_1000.pcap:udp"]["counts"]
    cand = hits[relations[0][0]] & hits[relations[0][1]]
    assert 0 < rows[0].sum() < cand.sum()
    try:
        reset(gm)
        gm.set_patterns(tokens)
        for how in ("arena", "frames"):
            if how == "arena":
                gm.load_arena(arena)
            else:
                assert gm.load_pcap_frames(os.path.join(DATA, "udp_1000.pcap"), "udp")[0] == len(payloads)
            gm.set_relations(relations)
            for _, kernel, fused in KERNELS:
                gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
                check_relations(gm, rows, counts)
            reset(gm)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 12. the command lines: KMPGPU_RELATIONS_FILE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"]), ("openmp_data", ["3"])])
def test_cli_relations_file(tokens, tmp_path, capture, prog, extra):
    _, payloads, relations, hits, rows = capture
    n = len(tokens)
    text = "# a b dmin dmax\n\n" + "".join(f"{a} {b} {'*' if lo is None else lo} {'*' if hi is None else hi}\n" for a, b, lo, hi in relations)
    lf = tmp_path / "relations.txt"
    lf.write_text(text)
    a0, b0 = relations[0][0], relations[0][1]
    rules = [([a0, b0, n + 0], []), ([a0], [n + 0]), ([n + 1], []), ([], [n + 2, a0]), ([n + 0, n + 1], [])]
    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([str(i) if i < n else f"r{i - n}" for i in pos] + [f"!{i}" if i < n else f"!r{i - n}" for i in neg]) + "\n" for pos, neg in rules))
    al = tmp_path / "alerts.csv"
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RELATIONS_FILE": str(lf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        assert strip_elapsed(r.stdout) == f.read()
    got = [tuple(int(x) for x in line.split(",")) for line in al.read_text().splitlines()]
    want = MM.rule_rows(np.concatenate([hits, rows]), rules)
    assert got == sorted((int(k), int(r_)) for r_, k in np.argwhere(want))
    assert want[0].any() and want[1].any()
    # a relations file that does not parse, a missing one, or the variable without its partners: exit 1 before any GPU work
    bad = tmp_path / "bad.txt"
    bad.write_text("0 1 0 5\n0 1 9 3\n")
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RELATIONS_FILE": str(bad), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 1 and "line 2: " in r.stderr and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RELATIONS_FILE": str(tmp_path / "none.txt"), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 1 and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RELATIONS_FILE": str(lf)})
    assert r.returncode == 1 and "KMPGPU_RULES_FILE" in r.stderr and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RELATIONS_FILE": str(lf), "KMPGPU_RULES_FILE": str(rf)})
    assert r.returncode == 1 and "KMPGPU_ALERTS_FILE" in r.stderr and r.stdout == ""
    # without the relations the same rules file does not parse: r0 is no term
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 1 and "line 1: " in r.stderr and r.stdout == ""
