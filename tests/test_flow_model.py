"""tests/flow_model.py held to hand-written cases and to the committed captures: the figures below are counted here with the pure-Python
pcap reader and extractor of tests/header_model.py, and everything the GPU tests compare flows with rests on them.  No GPU needed."""
import os

import numpy as np
import pytest

from conftest import DATA

import flow_model as FM
import header_model as HM

A, B, C = 0x0A000001, 0x0A000002, 0xC0A80101

# (capture, mode): payloads, directed flows, bidirectional flows, payloads of the largest bidirectional flow
FIXTURES = {
    ("big_udp.pcap", "udp"): (3358, 1630, 836, 415),
    ("very_big_udp.pcap", "udp"): (13768, 7281, 3641, 58),
    ("udp_1000.pcap", "udp"): (321, 45, 45, 89),
    ("udp_1000.pcap", "tcp"): (20, 4, 3, 10),
    ("tcp.pcap", "tcp"): (13, 2, 1, 13),
    ("udp.pcap", "udp"): (20, 5, 5, 8),
}


def _meta(*recs):
    return HM.meta_array(list(recs))


def test_two_directions_are_one_flow_unless_directed():
    meta = _meta((A, B, 1000, 80, 6), (B, A, 80, 1000, 6), (A, B, 1000, 80, 6), (C, A, 5, 6, 17))
    assert FM.flow_of(meta).tolist() == [0, 0, 0, 1]
    assert FM.flow_of(meta, directed=True).tolist() == [0, 1, 0, 2]
    recs = FM.records(meta, [10, 20, 30, 40])
    assert recs["first_packet"].tolist() == [0, 3] and recs["last_packet"].tolist() == [2, 3]
    assert recs["n_packets"].tolist() == [3, 1] and recs["payload_bytes"].tolist() == [60, 40]
    # the flow's direction is its first payload's
    assert recs["first"].tobytes() == meta[[0, 3]].tobytes()
    recs = FM.records(meta, [10, 20, 30, 40], directed=True)
    assert recs["first_packet"].tolist() == [0, 1, 3] and recs["last_packet"].tolist() == [2, 1, 3] and recs["payload_bytes"].tolist() == [40, 20, 40]


def test_keys_that_differ_in_one_field():
    base = (A, B, 1000, 80, 6)
    others = [(C, B, 1000, 80, 6), (A, C, 1000, 80, 6), (A, B, 1001, 80, 6), (A, B, 1000, 81, 6), (A, B, 1000, 80, 17)]
    for directed in (False, True):
        assert FM.flow_of(_meta(base, *others, base), directed).tolist() == [0, 1, 2, 3, 4, 5, 0]


def test_swapped_ports_are_another_flow():
    # A:1 -> B:2 against A:2 -> B:1: the endpoints differ, whatever the direction
    meta = _meta((A, B, 1, 2, 17), (A, B, 2, 1, 17), (B, A, 2, 1, 17), (B, A, 1, 2, 17))
    assert FM.flow_of(meta).tolist() == [0, 1, 0, 1]
    assert FM.flow_of(meta, directed=True).tolist() == [0, 1, 2, 3]
    # one address on both sides: the ports alone order the endpoints
    meta = _meta((A, A, 1, 2, 17), (A, A, 2, 1, 17))
    assert FM.flow_of(meta).tolist() == [0, 0]
    assert FM.flow_of(meta, directed=True).tolist() == [0, 1]


def test_reserved_is_not_part_of_the_key():
    meta = _meta((A, B, 1, 2, 17), (A, B, 1, 2, 17))
    meta["reserved"][1] = (1, 2, 3)
    assert FM.flow_of(meta).tolist() == [0, 0]
    assert FM.records(meta, [1, 1])["first"].tobytes() == meta[:1].tobytes()


def test_numbering_follows_the_first_payload():
    meta = _meta((C, A, 9, 9, 17), (A, B, 1, 2, 17), (C, A, 9, 9, 17), (B, C, 3, 4, 6), (A, B, 1, 2, 17))
    assert FM.flow_of(meta).tolist() == [0, 1, 0, 2, 1]


def test_fold_rules_and_expand():
    fo = np.array([0, 1, 0, 2, 1, 2], dtype=np.uint32)
    rows = np.array([[1, 0, 0, 0, 0, 0],          # A in payload 0 (flow 0)
                     [0, 0, 1, 0, 1, 0],          # B in payloads 2 (flow 0) and 4 (flow 1)
                     [0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 1]], dtype=bool)
    assert FM.fold(rows, fo).astype(int).tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 0], [0, 0, 1]]
    rules = [([0, 1], []), ([1], [0]), ([], [0, 1]), ([], [2])]
    # A and B meet in flow 0 though in no payload; flow 1 has B without A; flow 2 has neither; nothing holds row 2
    assert FM.flow_rules(rows, fo, rules).astype(int).tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]]
    assert FM.expand([True, False, True], fo).astype(int).tolist() == [1, 0, 1, 1, 0, 1]
    assert FM.fold(rows[:, :0], fo[:0]).shape == (4, 0)


def test_the_files_of_the_command_lines():
    meta = _meta((A, B, 1000, 80, 6), (B, A, 80, 1000, 6), (C, A, 5, 6, 17))
    recs = FM.records(meta, [10, 20, 40])
    assert FM.flows_file(recs) == "0,6,10.0.0.1,1000,10.0.0.2,80,0,1,2,30\n1,17,192.168.1.1,5,10.0.0.1,6,2,2,1,40\n"
    assert FM.flow_alerts_file(np.array([[0, 1], [1, 1]], dtype=bool)) == "0,1\n1,0\n1,1\n"


@pytest.mark.parametrize("pcap,mode", sorted(FIXTURES))
def test_fixture_flows(pcap, mode):
    n, directed, bidir, largest = FIXTURES[(pcap, mode)]
    pay, meta = HM.capture(HM.pcap_frames(os.path.join(DATA, pcap)), mode)
    assert len(pay) == n
    lens = [len(t) for t in pay]
    for d, want in ((True, directed), (False, bidir)):
        fo = FM.flow_of(meta, d)
        recs = FM.records(meta, lens, d)
        assert len(recs) == want == int(fo.max()) + 1
        assert int(recs["n_packets"].sum()) == n and int(recs["payload_bytes"].sum()) == sum(lens)
        assert np.array_equal(recs["n_packets"], np.bincount(fo))
        # numbered in the order of their first payload
        assert np.all(np.diff(recs["first_packet"].astype(np.int64)) > 0) and np.all(recs["first_packet"] <= recs["last_packet"])
    assert int(FM.records(meta, lens)["n_packets"].max()) == largest
    if (pcap, mode) == ("udp_1000.pcap", "tcp"):
        assert sorted(set(meta["proto"].tolist())) == [6, 17]         # the protocol byte keeps them apart


# ------------------------------------------------------------------------------------------------
# the vectorised model (flow_of_np, records_np) against the dict model, byte for byte
# ------------------------------------------------------------------------------------------------
def _same_as_the_dict_model(meta, lens):
    for directed in (False, True):
        fo = FM.flow_of_np(meta, directed)
        assert fo.dtype == np.uint32 and np.array_equal(fo, FM.flow_of(meta, directed))
        recs = FM.records_np(meta, lens, directed)
        assert recs.dtype == FM.FLOW_DTYPE and recs.tobytes() == FM.records(meta, lens, directed).tobytes()


def test_vectorised_model_on_the_hand_written_cases():
    base = (A, B, 1000, 80, 6)
    cases = [
        [(A, B, 1000, 80, 6), (B, A, 80, 1000, 6), (A, B, 1000, 80, 6), (C, A, 5, 6, 17)],
        [base, (C, B, 1000, 80, 6), (A, C, 1000, 80, 6), (A, B, 1001, 80, 6), (A, B, 1000, 81, 6), (A, B, 1000, 80, 17), base],
        [(A, B, 1, 2, 17), (A, B, 2, 1, 17), (B, A, 2, 1, 17), (B, A, 1, 2, 17)],
        [(A, A, 1, 2, 17), (A, A, 2, 1, 17)],
        [(C, A, 9, 9, 17), (A, B, 1, 2, 17), (C, A, 9, 9, 17), (B, C, 3, 4, 6), (A, B, 1, 2, 17)],
        [(0, 0, 0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 65535, 65535, 255), (0, 0xFFFFFFFF, 0, 65535, 0), (0xFFFFFFFF, 0, 65535, 0, 0)],
        [base],
        [],
    ]
    for recs in cases:
        meta = _meta(*recs)
        _same_as_the_dict_model(meta, [10 * (k + 1) for k in range(len(recs))])
    # `reserved` is no part of the key, and travels with the first payload's record
    meta = _meta(base, base, (B, A, 80, 1000, 6))
    meta["reserved"][0] = (7, 0, 0)
    meta["reserved"][2] = (0, 0, 9)
    _same_as_the_dict_model(meta, [1, 2, 3])
    assert FM.flow_of_np(meta).tolist() == [0, 0, 0] and FM.records_np(meta, [1, 2, 3])["first"].tobytes() == meta[:1].tobytes()
    assert FM.flow_of_np(meta[:0]).shape == (0,) and FM.records_np(meta[:0], []).shape == (0,)


@pytest.mark.parametrize("pcap,mode", sorted(FIXTURES))
def test_vectorised_model_on_the_fixtures(pcap, mode):
    n, directed, bidir, _ = FIXTURES[(pcap, mode)]
    pay, meta = HM.capture(HM.pcap_frames(os.path.join(DATA, pcap)), mode)
    _same_as_the_dict_model(meta, [len(t) for t in pay])
    assert len(FM.records_np(meta, [len(t) for t in pay], True)) == directed and int(FM.flow_of_np(meta).max()) + 1 == bidir


@pytest.mark.parametrize("seed,n,n_keys", [(1, 5000, 40), (2, 3000, 700), (3, 4001, 4001)])
def test_vectorised_model_on_random_records(seed, n, n_keys):
    """a few thousand records over few keys, so that most payloads join a flow that exists, in both directions; the fields are drawn
    from small domains, so that keys differ in one field only and the swap of an undirected key meets another flow's key"""
    rng = np.random.default_rng(seed)
    pool = HM.meta_array([(int(rng.choice([A, B, C, 0, 0xFFFFFFFF])), int(rng.choice([A, B, C, 0xFFFFFFFF])), int(rng.choice([0, 1, 80, 65535])),
                           int(rng.choice([0, 1, 80, 65535])) if n_keys < 1000 else int(rng.integers(1 << 16)), int(rng.choice([6, 17, 255]))) for _ in range(n_keys)])
    meta = pool[rng.integers(0, n_keys, n)]
    back = rng.random(n) < 0.4                         # the answer: source and destination swapped
    meta["src_ip"][back], meta["dst_ip"][back] = meta["dst_ip"][back], meta["src_ip"][back]
    meta["src_port"][back], meta["dst_port"][back] = meta["dst_port"][back], meta["src_port"][back]
    meta["reserved"] = rng.integers(0, 256, (n, 3))
    lens = rng.integers(0, 70000, n)
    _same_as_the_dict_model(meta, lens)
    assert len(FM.records_np(meta, lens, True)) > len(FM.records_np(meta, lens)) > 1
