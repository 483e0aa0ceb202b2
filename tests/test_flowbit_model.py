"""tests/flowbit_model.py against verdicts written by hand from the definition of include/kmpgpu.h ("flow bits"): the model is what the
GPU tests hold kmpgpu_scan_flowbits to, so it is held to cases small enough to decide on paper.  No GPU.
"""
import numpy as np

import flow_model as FM
import flowbit_model as FB
import header_model as HM


def bits(s):
    return [c == "1" for c in s.replace(" ", "")]


def base_of(*rows):
    return np.array([bits(r) for r in rows], dtype=bool)


def rows_of(a):
    return ["".join("1" if x else "0" for x in r) for r in a]


ONE = [0] * 8


def test_login_then_command():
    # rule 0: USER, sets bit 0 and does not alert; rule 1: the command, alerts only where a login was seen BEFORE the payload
    ops = [(0, "set", 0), (0, "noalert"), (1, "isset", 0)]
    #                login at 2      command at 1, 2, 5: payload 2 holds both -- the tester does not fire there
    base = base_of("00100000", "01100100")
    got = FB.run(base, ONE, ops, 1)
    assert rows_of(got["alert"]) == ["00000000", "00000100"]
    assert rows_of(got["fired"]) == ["00100000", "00000100"]
    assert rows_of(got["state"]) == ["00011111"]
    assert got["flow_state"].tolist() == [1]


def test_fire_once():
    ops = [(0, "isnotset", 0), (0, "set", 0)]
    got = FB.run(base_of("01101101"), ONE, ops, 1)
    assert rows_of(got["alert"]) == ["01000000"]
    assert rows_of(got["state"]) == ["00111111"]


def test_unset_stops_the_alerts():
    # rule 0 logs in, rule 1 is the command, rule 2 the logout
    ops = [(0, "set", 0), (0, "noalert"), (1, "isset", 0), (2, "unset", 0), (2, "noalert")]
    base = base_of("10000100", "01111111", "00010000")
    got = FB.run(base, ONE, ops, 1)
    #                           state before: 0 1 1 1 0 0 1 1
    assert rows_of(got["state"]) == ["01110011"]
    assert rows_of(got["alert"]) == ["00000000", "01110011", "00000000"]
    assert got["flow_state"].tolist() == [1]


def test_toggle_twice():
    got = FB.run(base_of("11011000"), ONE, [(0, "toggle", 0)], 1)
    assert rows_of(got["state"]) == ["01001000"]
    assert got["flow_state"].tolist() == [0]
    # two toggles in one rule are none
    got = FB.run(base_of("11011000"), ONE, [(0, "toggle", 0), (0, "toggle", 0)], 1)
    assert rows_of(got["state"]) == ["00000000"]


def test_two_rules_on_one_bit_in_one_payload():
    # index order decides: rule 0 sets, rule 1 unsets -> clear; the other way round -> set
    both = base_of("00100000", "00100000")
    got = FB.run(both, ONE, [(0, "set", 0), (1, "unset", 0)], 1)
    assert rows_of(got["state"]) == ["00000000"]
    got = FB.run(both, ONE, [(0, "unset", 0), (1, "set", 0)], 1)
    assert rows_of(got["state"]) == ["00011111"]
    # ... and not the order the ops were given in
    got = FB.run(both, ONE, [(1, "set", 0), (0, "unset", 0)], 1)
    assert rows_of(got["state"]) == ["00011111"]
    # inside one rule the order given does
    got = FB.run(both[:1], ONE, [(0, "set", 0), (0, "unset", 0)], 1)
    assert rows_of(got["state"]) == ["00000000"]
    got = FB.run(both[:1], ONE, [(0, "unset", 0), (0, "set", 0)], 1)
    assert rows_of(got["state"]) == ["00011111"]


def test_noalert_fires_and_acts():
    got = FB.run(base_of("10100000"), ONE, [(0, "noalert"), (0, "toggle", 0)], 1)
    assert rows_of(got["alert"]) == ["00000000"] and rows_of(got["fired"]) == ["10100000"]
    assert rows_of(got["state"]) == ["01100000"]


def test_interleaved_flows_share_nothing():
    ops = [(0, "isnotset", 0), (0, "set", 0)]
    flow = [0, 1, 0, 1, 2, 1, 0, 2]
    got = FB.run(base_of("11111111"), flow, ops, 1)
    assert rows_of(got["alert"]) == ["11001000"]
    assert rows_of(got["state"]) == ["00110111"]
    assert got["flow_state"].tolist() == [1, 1, 1]


def test_directed_against_undirected():
    # a request sets the bit, the answer tests it: one state where both directions are one flow, two where they are not
    A, B = 0x0A000001, 0x0A000002
    meta = HM.meta_array([(A, B, 1000, 80, 6), (B, A, 80, 1000, 6), (A, B, 1000, 80, 6), (B, A, 80, 1000, 6)])
    ops = [(0, "set", 0), (0, "noalert"), (1, "isset", 0)]
    base = base_of("1010", "0101")
    got = FB.run(base, FM.flow_of(meta), ops, 1)
    assert rows_of(got["alert"]) == ["0000", "0101"] and got["flow_state"].tolist() == [1]
    got = FB.run(base, FM.flow_of(meta, directed=True), ops, 1)
    assert rows_of(got["alert"]) == ["0000", "0000"] and got["flow_state"].tolist() == [1, 0]


def test_three_levels():
    # bit 0 -> bit 1 -> bit 2: every stage needs the one before it to have happened in an EARLIER payload
    ops = [(0, "set", 0), (1, "isset", 0), (1, "set", 1), (2, "isset", 1), (2, "set", 2), (3, "isset", 2)]
    assert FB.levels(ops, 3) == [0, 1, 2]
    base = base_of("01000000", "01100000", "01110000", "01111000")
    got = FB.run(base, ONE, ops, 3)
    assert rows_of(got["state"]) == ["00111111", "00011111", "00001111"]
    assert rows_of(got["alert"]) == ["01000000", "00100000", "00010000", "00001000"]
    assert got["flow_state"].tolist() == [7]
    # a rule may test the bit it changes: no edge, no level
    assert FB.levels([(0, "isnotset", 0), (0, "set", 0)], 1) == [0]
    assert FB.levels([(0, "isset", 0), (0, "set", 1), (1, "isset", 1), (1, "set", 0)], 2) is None
