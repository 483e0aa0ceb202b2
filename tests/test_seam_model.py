"""tests/seam_model.py against hand-written cases, against itself (the loop form and the numpy form) and against the property the
seams exist for: on whole payloads, a pattern of at most reach + 1 bytes occurs across a boundary of a flow direction's concatenated
stream iff it occurs in that boundary's seam."""
import numpy as np
import pytest

import flow_model as FM
import match_model as MM
import seam_model as SM
from header_model import META_DTYPE

A, B, C_ = 0x0A000001, 0x0A000002, 0x0A000003


def meta_of(rows):
    """(src_ip, src_port, dst_ip, dst_port) per payload, UDP"""
    m = np.zeros(len(rows), dtype=META_DTYPE)
    for k, (s, sp, d, dp) in enumerate(rows):
        m[k]["src_ip"], m[k]["src_port"], m[k]["dst_ip"], m[k]["dst_port"], m[k]["proto"] = s, sp, d, dp, 17
    return m


def as_tuples(recs):
    return [(int(r["prev"]), int(r["next"]), int(r["tail_len"]), int(r["head_len"])) for r in recs]


def test_one_flow_one_direction():
    meta = meta_of([(A, 1, B, 2)] * 3)
    pay = [b"GET /adm", b"in HTTP/1.1 and more", b""]
    recs = SM.records(meta, [len(p) for p in pay], reach=4)
    assert as_tuples(recs) == [(0, 1, 4, 4), (1, 2, 4, 0)]
    assert SM.payloads(pay, recs) == [b"/admin H", b"more"]
    # a reach beyond both payloads takes them whole
    recs = SM.records(meta, [len(p) for p in pay], reach=98)
    assert as_tuples(recs) == [(0, 1, 8, 20), (1, 2, 20, 0)]
    assert SM.payloads(pay, recs) == [b"GET /admin HTTP/1.1 and more", b"in HTTP/1.1 and more"]


def test_two_directions_are_two_chains():
    # payloads 0, 2, 3 run A -> B, payloads 1, 4 run B -> A: one flow, two chains
    meta = meta_of([(A, 1, B, 2), (B, 2, A, 1), (A, 1, B, 2), (A, 1, B, 2), (B, 2, A, 1)])
    fo = FM.flow_of(meta)
    assert fo.tolist() == [0] * 5
    assert SM.direction(meta, fo).tolist() == [0, 1, 0, 0, 1]
    assert SM.pred(fo, SM.direction(meta, fo)).tolist() == [-1, -1, 0, 2, 1]
    assert as_tuples(SM.records(meta, [5] * 5, reach=3)) == [(0, 2, 3, 3), (2, 3, 3, 3), (1, 4, 3, 3)]
    # directed: two flows, every payload's dir is 0
    fo = FM.flow_of(meta, directed=True)
    assert fo.tolist() == [0, 1, 0, 0, 1]
    assert SM.direction(meta, fo).tolist() == [0] * 5
    assert as_tuples(SM.records(meta, [5] * 5, reach=3, directed=True)) == [(0, 2, 3, 3), (2, 3, 3, 3), (1, 4, 3, 3)]


def test_equal_endpoints_have_one_direction():
    meta = meta_of([(A, 7, A, 7)] * 3)
    fo = FM.flow_of(meta)
    assert SM.direction(meta, fo).tolist() == [0, 0, 0]
    assert as_tuples(SM.records(meta, [1, 0, 2], reach=98)) == [(0, 1, 1, 0), (1, 2, 0, 2)]


def test_interleaved_flows_and_empty_seams():
    meta = meta_of([(A, 1, B, 2), (C_, 1, B, 2), (A, 1, B, 2), (C_, 1, B, 2)])
    pay = [b"", b"xy", b"", b"z"]
    recs = SM.records(meta, [len(p) for p in pay], reach=16)
    assert as_tuples(recs) == [(0, 2, 0, 0), (1, 3, 2, 1)]
    seams = SM.payloads(pay, recs)
    assert seams == [b"", b"xyz"]
    arena, off, ln = SM.arena(seams)
    assert off.tolist() == [0, 16] and ln.tolist() == [0, 3]          # an empty seam owns one zero slot
    assert bytes(arena) == b"\0" * 16 + b"xyz" + b"\0" * 13


def test_single_payload_flows_have_no_seam():
    meta = meta_of([(A, k, B, 2) for k in range(5)])
    assert len(SM.records(meta, [9] * 5, reach=98)) == 0
    assert len(SM.records_np(meta, [9] * 5, reach=98)) == 0
    assert len(SM.records_np(meta[:0], [], reach=98)) == 0


def random_capture(rng, n, n_flows, lens):
    flow = rng.integers(0, n_flows, n)
    back = rng.integers(0, 3, n) == 0
    rows = [((B, 53, A + f, 1000 + f % 7) if b else (A + f, 1000 + f % 7, B, 53)) for f, b in zip(flow.tolist(), back.tolist())]
    ln = rng.choice(lens, n)
    pay = [bytes(rng.integers(97, 101, int(x), dtype=np.uint8)) for x in ln]            # a four-letter alphabet: patterns do occur
    return meta_of(rows), pay


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("reach", [1, 15, 16, 98])
def test_identity_and_numpy_form(directed, reach):
    rng = np.random.default_rng(reach + 100 * directed)
    meta, pay = random_capture(rng, 400, 40, [0, 1, 15, 16, 17, reach - 1 if reach > 1 else 2, reach, reach + 1, 200])
    lens = [len(p) for p in pay]
    fo = FM.flow_of(meta, directed)
    dr = SM.direction(meta, fo)
    recs = SM.records(meta, lens, reach, directed)
    # n_seams == n_pkts - #(flow, dir)
    assert len(recs) == len(pay) - len({(int(f), int(d)) for f, d in zip(fo, dr)})
    assert np.all(recs["next"][1:] > recs["next"][:-1])
    assert np.array_equal(SM.records_np(meta, lens, reach, directed), recs)
    for r, s in zip(recs, SM.payloads(pay, recs)):
        assert len(s) == int(r["tail_len"]) + int(r["head_len"]) <= 2 * reach
        assert fo[int(r["prev"])] == fo[int(r["next"])] and dr[int(r["prev"])] == dr[int(r["next"])] and int(r["prev"]) < int(r["next"])


@pytest.mark.parametrize("reach", [1, 3, 7, 16])
def test_stream_property_whole_payloads(reach):
    """Every payload at least `reach` bytes long: a pattern of m <= reach + 1 bytes starts at stream offset s with s < boundary < s + m
    (it straddles that boundary, and no other: m - 1 <= reach <= every length) iff it occurs in the boundary's seam, which holds exactly
    the stream's bytes [boundary - reach, boundary + reach)."""
    rng = np.random.default_rng(reach)
    meta, pay = random_capture(rng, 120, 6, [reach, reach + 1, reach + 5, 40])
    pay = [p if rng.integers(0, 4) else p[: len(p) // 2] + b"\0" + p[len(p) // 2 + 1:] for p in pay]         # whole payloads: a 0x00 is a byte
    pay = [p if len(p) >= reach else p + b"a" * (reach - len(p)) for p in pay]
    lens = [len(p) for p in pay]
    fo = FM.flow_of(meta)
    dr = SM.direction(meta, fo)
    recs = SM.records(meta, lens, reach)
    seams = SM.payloads(pay, recs)
    pats = [bytes(rng.integers(97, 101, int(m), dtype=np.uint8)) for m in rng.integers(1, reach + 2, 24)]
    st = MM.starts(seams, pats, whole=True)
    seam_of = {int(r["next"]): j for j, r in enumerate(recs)}
    checked = across_seen = 0
    for chain in {(int(f), int(d)) for f, d in zip(fo, dr)}:
        ks = [k for k in range(len(pay)) if (int(fo[k]), int(dr[k])) == chain]
        stream = b"".join(pay[k] for k in ks)
        bounds = np.cumsum([lens[k] for k in ks])[:-1]
        for k, b in zip(ks[1:], bounds.tolist()):
            j = seam_of[k]
            assert seams[j] == stream[b - reach:b + reach]
            for i, p in enumerate(pats):
                m = len(p)
                across = any(stream[s:s + m] == p for s in range(b - m + 1, b))
                # across the boundary in the stream iff across the junction in the seam (the seam may also hold the pattern on one side of
                # its junction: that is a match inside prev or next, which the stream holds too)
                assert across == any(s < reach < s + m for s in st[j][i]), (chain, k, p)
                assert all(stream[b - reach + s:b - reach + s + m] == p for s in st[j][i])
                checked += 1
                across_seen += across
    assert checked > 500 and across_seen > 5


def test_combined_terms_take_seam_bits_in_pattern_rows_only():
    fo = np.array([0, 1, 0, 1], dtype=np.uint32)
    src_terms = np.zeros((3, 4), dtype=bool)             # two patterns and one further term (a header predicate, say)
    src_terms[2, 1] = True
    seam_hits = np.array([[True, False], [False, False]])
    seam_flow = np.array([0, 1], dtype=np.uint32)
    terms = SM.combined_terms(src_terms, seam_hits, fo, seam_flow, 2)
    assert terms.tolist() == [[True, False], [False, False], [False, True]]
    rows = SM.flow_rules(src_terms, seam_hits, fo, seam_flow, [([0], [1]), ([0, 2], [])], 2)
    assert rows.tolist() == [[True, False], [False, False]]
    # no seams: the fold of flow_model
    none = np.zeros((2, 0), dtype=bool)
    assert np.array_equal(SM.combined_terms(src_terms, none, fo, seam_flow[:0], 2), FM.fold(src_terms, fo, 2))
