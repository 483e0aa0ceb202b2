"""tests/stream_seq_model.py held to hand-written cases, its cell formulation to the running maximum the kernels use on 20 000 random small
streams, and matcher.stream_locate_ordered to the model's origins.  No GPU."""
import numpy as np
import pytest

import stream_seq_model as QM
from header_model import META_DTYPE
from multithreading_string_matching_amd.matcher import STREAM_ORDER_DTYPE, STREAM_SEG_DTYPE, stream_locate_ordered

A, B = 0x0A000001, 0xC0A80101
X, Y, Z = (A, 40000, B, 80), (B, 80, A, 40000), (A + 1, 40001, B, 80)
DEPTH = 1 << 20


def _meta(rows, proto=6):
    m = np.zeros(len(rows), dtype=META_DTYPE)
    for k, (s, sp, d, dp) in enumerate(rows):
        m[k]["src_ip"], m[k]["src_port"], m[k]["dst_ip"], m[k]["dst_port"], m[k]["proto"] = s, sp, d, dp, proto
    return m


def _one(pay, seq, depth=DEPTH):
    """one TCP stream of one direction"""
    streams, recs, pos, segs, orders, origin = QM.build(pay, _meta([X] * len(pay)), seq, depth)
    assert len(streams) == 1
    return streams[0], recs[0], pos, segs, orders[0]


def test_the_dtypes_are_the_librarys():
    assert QM.SEG_DTYPE == STREAM_SEG_DTYPE and STREAM_SEG_DTYPE.itemsize == 16
    assert QM.ORDER_DTYPE == STREAM_ORDER_DTYPE and STREAM_ORDER_DTYPE.itemsize == 32


def test_in_order_is_concatenation():
    data, r, pos, segs, o = _one([b"GET ", b"/adm", b"in"], [1000, 1004, 1008])
    assert data == b"GET /admin" and pos["pos"].tolist() == [0, 4, 8]
    assert segs["skip"].tolist() == [0, 0, 0] and segs["take"].tolist() == [4, 4, 2] and segs["seq_off"].tolist() == [0, 4, 8]
    assert (o["seq_base"], o["n_gaps"], o["gap_bytes"], o["dup_bytes"], o["tcp"]) == (1000, 0, 0, 0, 1)


def test_reordered_segments():
    data, r, pos, segs, o = _one([b"in", b"GET ", b"/adm"], [1008, 1000, 1004])
    assert data == b"GET /admin" and pos["pos"].tolist() == [8, 0, 4]
    assert (r["first_packet"], r["last_packet"], r["n_packets"], r["bytes"]) == (0, 2, 3, 10)        # capture order
    assert segs["seq_off"].tolist() == [8, 0, 4] and o["seq_base"] == 1000 and o["n_gaps"] == 0


def test_exact_retransmission():
    data, r, pos, segs, o = _one([b"abcd", b"efgh", b"efgh", b"ij"], [10, 14, 14, 18])
    assert data == b"abcdefghij" and r["bytes"] == 10
    assert segs["skip"].tolist() == [0, 0, 4, 0] and segs["take"].tolist() == [4, 4, 0, 2]
    assert pos["pos"].tolist() == [0, 4, 8, 8]                  # the covered member sits where the next byte goes
    assert (o["dup_bytes"], o["n_gaps"], o["gap_bytes"]) == (4, 0, 0)


@pytest.mark.parametrize("skip", [1, 5, 17])
def test_partial_overlap(skip):
    first, second = bytes(range(1, 31)), bytes(range(101, 131))
    data, r, pos, segs, o = _one([first, second], [500, 500 + 30 - skip])
    assert data == first + second[skip:]
    assert segs["skip"].tolist() == [0, skip] and segs["take"].tolist() == [30, 30 - skip] and pos["pos"].tolist() == [0, 30]
    assert o["dup_bytes"] == skip


def test_a_longer_segment_with_the_same_sequence_number_captured_second():
    data, r, pos, segs, o = _one([b"abc", b"ABCDEF"], [7, 7])
    assert data == b"abcDEF"                                    # equal sequence numbers stay in capture order: the first one wins
    assert segs["skip"].tolist() == [0, 3] and segs["take"].tolist() == [3, 3] and pos["pos"].tolist() == [0, 3]


def test_the_first_captured_member_is_not_the_lowest():
    data, r, pos, segs, o = _one([b"world", b"hello "], [106, 100])
    assert data == b"hello world" and segs["seq_off"].tolist() == [6, 0] and o["seq_base"] == 100
    assert QM.rel(100, 106) == -6


def test_sequence_numbers_crossing_2_32():
    data, r, pos, segs, o = _one([b"bbbb", b"cccc", b"aaaa"], [0xFFFFFFFE, 2, 0xFFFFFFFA])
    assert data == b"aaaabbbbcccc" and segs["seq_off"].tolist() == [4, 8, 0] and o["seq_base"] == 0xFFFFFFFA
    assert o["n_gaps"] == 0 and o["dup_bytes"] == 0


def test_a_zero_length_member():
    data, r, pos, segs, o = _one([b"ab", b"", b"cd", b""], [0, 2, 2, 1])
    assert data == b"abcd" and pos["pos"].tolist() == [0, 2, 2, 2] and segs["take"].tolist() == [2, 0, 2, 0]
    assert segs["seq_off"].tolist() == [0, 2, 2, 1] and o["n_gaps"] == 0


def test_a_gap():
    data, r, pos, segs, o = _one([b"abc", b"xyz", b"q"], [0, 10, 30])
    assert data == b"abcxyzq" and pos["pos"].tolist() == [0, 3, 6]                # holes closed
    assert (o["n_gaps"], o["gap_bytes"], o["dup_bytes"]) == (2, 7 + 17, 0)
    # a SYN's phantom byte is a 1-byte gap
    data, r, pos, segs, o = _one([b"", b"GET"], [99, 100])
    assert data == b"GET" and (o["n_gaps"], o["gap_bytes"]) == (1, 1)


def test_the_cut():
    data, r, pos, segs, o = _one([b"efgh", b"abcd", b"abcd"], [4, 0, 0], depth=6)
    assert data == b"abcdef" and (r["bytes"], r["len"]) == (8, 6)
    assert segs["take"].tolist() == [4, 4, 0] and pos["pos"].tolist() == [4, 0, 4]                  # before the cut


def test_a_udp_flow_beside_a_tcp_flow():
    pay = [b"22", b"bb", b"11", b"aa", b"22"]
    meta = _meta([X, Z, X, Z, X])
    meta["proto"][[1, 3]] = 17
    seq = [5, 9, 3, 1, 5]                                       # Z's are not sequence numbers: capture order
    streams, recs, pos, segs, orders, origin = QM.build(pay, meta, seq, DEPTH)
    assert streams == [b"1122", b"bbaa"]
    assert orders["tcp"].tolist() == [1, 0] and orders["dup_bytes"].tolist() == [2, 0] and orders["seq_base"].tolist() == [3, 0]
    assert segs["skip"].tolist() == [0, 0, 0, 0, 2] and segs["seq_off"].tolist() == [2, 0, 0, 0, 2]
    assert pos["pos"].tolist() == [2, 0, 0, 2, 4]
    assert origin[0] == [(2, 0), (2, 1), (0, 0), (0, 1)]


def test_the_two_formulations_agree_on_random_streams():
    rng = np.random.default_rng(1)
    for _ in range(20000):
        m = int(rng.integers(1, 7))
        lens = rng.integers(0, 6, m)
        start = int(rng.choice([0, 1000, 0xFFFFFFF8, 0x7FFFFFFC]))
        seq = (start + rng.integers(0, 12, m)) & 0xFFFFFFFF
        pay = [bytes(rng.integers(1, 256, int(x), dtype=np.uint8)) for x in lens]
        data, r, pos, segs, o = _one(pay, seq)
        order = sorted(range(m), key=lambda k: (int(segs[k]["seq_off"]), k))
        kept = QM.kept_by_maximum([len(pay[k]) for k in order], [int(segs[k]["seq_off"]) for k in order])
        assert kept == [(int(segs[k]["skip"]), int(segs[k]["take"])) for k in order]
        assert data == b"".join(pay[k][int(segs[k]["skip"]):] for k in order)
        at = 0
        for k, (skip, take) in zip(order, kept):
            assert int(pos[k]["pos"]) == at
            at += take
        assert at == int(r["bytes"]) and int(o["dup_bytes"]) == int(lens.sum()) - at


def test_stream_locate_ordered_against_the_origins():
    rng = np.random.default_rng(5)
    n = 300
    rows = [(A + int(f), 1000, B, 80) for f in rng.integers(0, 12, n)]
    meta = _meta(rows)
    meta["proto"][[k for k in range(n) if rows[k][0] % 4 == 0]] = 17
    pay = [bytes(rng.integers(1, 256, int(x), dtype=np.uint8)) for x in rng.integers(0, 9, n)]
    seq = rng.integers(0, 40, n).astype(np.uint32) + np.uint32(0xFFFFFFF0)
    streams, recs, pos, segs, orders, origin = QM.build(pay, meta, seq, DEPTH)
    st = np.concatenate([np.full(len(o), s) for s, o in enumerate(origin)])
    at = np.concatenate([np.arange(len(o)) for o in origin])
    k, j = stream_locate_ordered(pos, segs, st, at)
    assert list(zip(k.tolist(), j.tolist())) == [x for o in origin for x in o]
    with pytest.raises(ValueError, match="behind"):
        stream_locate_ordered(pos, segs, [0], [len(origin[0])])
