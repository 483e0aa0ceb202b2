"""tests/chain_model.py against the definition (an enumeration of all tuples) and against match_model.relation_rows: no GPU needed."""
import random

import numpy as np

import chain_model as CM
import match_model as MM


def _case(rng, max_contents=5):
    pats = [bytes(rng.choice(b"ab") for _ in range(rng.choice([1, 1, 2, 3]))) for _ in range(4)]
    payloads = []
    for _ in range(12):
        L = rng.choice([0, 1, 5, 11, 18])
        payloads.append(bytes(rng.choice(b"abc") if rng.random() < 0.2 else rng.choice(b"ab") for _ in range(L)))
    chains = []
    for _ in range(10):
        ch = [rng.randrange(4)]
        for _ in range(rng.randrange(1, max_contents)):
            lo = rng.randrange(-12, 12)
            ch.append((rng.randrange(4), None if rng.random() < 0.15 else lo, None if rng.random() < 0.15 else lo + rng.randrange(0, 9)))
        chains.append(tuple(ch))
    return pats, payloads, chains


def test_stage_by_stage_equals_all_tuples():
    rng = random.Random("chain-model")
    held = failed = 0
    for _ in range(60):
        pats, payloads, chains = _case(rng)
        st = MM.starts(payloads, pats)
        rows = CM.chain_rows(st, pats, chains)
        for c, chain in enumerate(chains):
            for k, row in enumerate(st):
                want = CM.chain_holds_all_tuples(row, pats, chain)
                assert rows[c, k] == want, (payloads[k], pats, chain)
                held += want
                failed += (not want) and all(row[p] for p, _, _ in CM.links(chain))
    assert held > 100 and failed > 100                 # both answers are exercised, the second on payloads that hold every content


def test_two_contents_are_the_relation():
    rng = random.Random("chain-model-2")
    for _ in range(40):
        pats, payloads, chains = _case(rng, max_contents=2)
        assert all(len(ch) == 2 for ch in chains)
        st = MM.starts(payloads, pats)
        rels = [CM.pairwise_relations(ch)[0] for ch in chains]
        assert np.array_equal(CM.chain_rows(st, pats, chains), MM.relation_rows(st, pats, rels))


def test_a_chain_asks_for_more_than_its_relations():
    """A .. B1 .. B2 .. C: (A, B1) and (B2, C) are in range, no single B serves both"""
    pats = [b"A", b"B", b"C"]
    chain = (0, (1, 0, 2), (2, 0, 2))
    two, one = b"A.B......B.C", b"A.B.C"
    st = MM.starts([two, one], pats)
    rel = MM.relation_rows(st, pats, CM.pairwise_relations(chain))
    assert rel.all()
    assert CM.chain_rows(st, pats, [chain]).tolist() == [[False, True]]


def test_repeats_and_self_pairing():
    pats = [b"ab"]
    st = MM.starts([b"ab", b"abab", b"ababab", b"ab...ab......ab"], pats)
    rows = CM.chain_rows(st, pats, [(0, (0, 0, 0), (0, 0, 0)), (0, (0, -2, -2), (0, -2, -2)), (0, (0, 0, None), (0, 0, None)), (0, (0, 9, 9))])
    assert rows.tolist() == [[False, False, True, False], [True] * 4, [False, False, True, True], [False, False, False, False]]
    # the nearest earlier match is out of range, an earlier one is in
    assert CM.chain_rows(st, pats, [(0, (0, 10, 12))]).tolist() == [[False, False, False, True]]


def test_flat_chains():
    off, flat = CM.flat_chains([(3, (1, None, 5)), (0, (0, -2, None), (2, 1, 1))])
    assert off.tolist() == [0, 2, 5]
    assert flat == [(3, MM.I32_MIN, MM.I32_MAX), (1, MM.I32_MIN, 5), (0, MM.I32_MIN, MM.I32_MAX), (0, -2, MM.I32_MAX), (2, 1, 1)]
