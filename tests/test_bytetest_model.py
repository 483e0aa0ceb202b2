"""tests/bytetest_model.py held to hand-written cases whose answers stand here, spelled out (no GPU, nothing of the library), and to the
DNS capture the byte tests were asked for."""
import os

import numpy as np
import pytest

import bytetest_model as BM
import header_model as HM
from bytetest_model import EQ, GE, GT, LE, LT, NE, bt
from conftest import DATA


def row(payload, test, whole=False, pats=(), windows=None, nocase=None):
    return bool(BM.bytetest_rows([payload], list(pats), [test], windows, nocase, whole)[0, 0])


def test_byte_orders_on_asymmetric_bytes():
    p = bytes([1, 2, 3, 4])
    assert row(p, bt(4, EQ, 0x01020304, 0))
    assert row(p, bt(4, EQ, 0x04030201, 0, little=True))
    assert not row(p, bt(4, EQ, 0x01020304, 0, little=True))
    assert not row(p, bt(4, EQ, 0x04030201, 0))
    assert row(p, bt(2, EQ, 0x0203, 1)) and row(p, bt(2, EQ, 0x0302, 1, little=True))
    assert row(p, bt(1, EQ, 3, 2)) and row(p, bt(1, EQ, 3, 2, little=True))


def test_three_byte_fields():
    p = bytes([1, 2, 3, 4])
    assert row(p, bt(3, EQ, 0x010203, 0)) and row(p, bt(3, EQ, 0x030201, 0, little=True))
    assert row(p, bt(3, EQ, 0x020304, 1)) and row(p, bt(3, EQ, 0x040302, 1, little=True))
    assert not row(p, bt(3, EQ, 0x020304, 0))
    assert not row(p, bt(3, GE, 0, 2))                    # bytes 2 .. 4 of a payload of 4


def test_compares_are_unsigned():
    p = bytes([0x80, 0, 0, 0, 1])
    assert row(p, bt(4, GT, 1, 0), whole=True) and not row(p, bt(4, LT, 1, 0), whole=True)
    assert row(p, bt(4, GE, 0x80000000, 0), whole=True) and row(p, bt(4, LE, 0x80000000, 0), whole=True)
    assert row(p, bt(1, GT, 0x7F, 0)) and not row(p, bt(1, LT, 0x7F, 0))
    for op, want in ((EQ, False), (NE, True), (LT, False), (GT, True), (LE, False), (GE, True)):
        assert row(b"\xFF\xFF\xFF\xFF", bt(4, op, 0x7FFFFFFF, 0)) == want, op


def test_mask():
    assert row(b"A", bt(1, EQ, 0, 0, mask=0)) and not row(b"A", bt(1, NE, 0, 0, mask=0))
    assert row(b"\x81\x80", bt(2, NE, 0, 0, mask=0x8000)) and not row(b"\x01\x80", bt(2, NE, 0, 0, mask=0x8000))      # the bit test "&"
    assert row(b"\x12\x34", bt(2, EQ, 0x0230, 0, mask=0x0FF0))
    assert not row(b"", bt(1, EQ, 0, 0, mask=0))          # mask 0 compares 0 with 0, but only where there is a field


def test_field_at_the_text_end():
    assert row(b"abcd", bt(2, EQ, 0x6364, 2))             # ends exactly at E_k = 4
    assert not row(b"abcd", bt(2, GE, 0, 3))              # one byte past it
    assert not row(b"abcd", bt(2, NE, 0x1234, 3))         # out of reach is false whatever the operator ...
    assert not row(b"abcd", bt(2, EQ, 0x1234, 3))         # ... so !b<q> fires on a payload that is too short
    assert row(b"abcd", BM.isdataat(3)) and not row(b"abcd", BM.isdataat(4))


def test_nul_inside_and_in_front_of_the_field():
    p = b"ab\0cd"
    for whole in (False, True):
        assert row(p, bt(1, EQ, 0x62, 1), whole)          # in front of the 0x00 under either rule
    assert not row(p, bt(2, EQ, 0x6200, 1)) and row(p, bt(2, EQ, 0x6200, 1), whole=True)          # the 0x00 inside the field
    assert not row(p, bt(1, EQ, 0x63, 3)) and row(p, bt(1, EQ, 0x63, 3), whole=True)              # the 0x00 in front of it
    assert not row(p, bt(1, EQ, 0, 2)) and row(p, bt(1, EQ, 0, 2), whole=True)                    # the 0x00 is the field
    assert not row(p, BM.isdataat(2)) and row(p, BM.isdataat(2), whole=True)
    assert not row(b"\0abc", bt(1, GE, 0, 0)) and row(b"\0abc", bt(1, GE, 0, 0), whole=True)      # E_k = 0


def test_short_payloads():
    pays = [b"", b"\x07", b"\x07\x08\x09", b"\x07\x08\x09\x0a"]                                    # L_k in {0, 1, 3, 4}
    tests = [bt(1, GE, 0, 0), bt(4, GE, 0, 0), bt(2, EQ, 0x0809, 1), bt(1, GE, 0, 3), bt(3, EQ, 0x090807, 0, little=True)]
    want = [[False, True, True, True], [False, False, False, True], [False, False, True, True], [False, False, False, True],
            [False, False, True, True]]
    assert BM.bytetest_rows(pays, [], tests).tolist() == want


def test_relative_offsets():
    pats = [b"LEN:"]
    p = b"xxLEN:\x01\x02yy"                                # the match: s = 2, its end: 6
    assert row(p, bt(2, EQ, 0x0102, 0, anchor=0), pats=pats)
    assert row(p, bt(2, EQ, 0x7979, 2, anchor=0), pats=pats)            # ends at E_k = 10
    assert not row(p, bt(2, GE, 0, 3, anchor=0), pats=pats)             # one past it
    assert row(p, bt(1, EQ, 0x3A, -1, anchor=0), pats=pats)             # into the match: its ':'
    assert row(p, bt(1, EQ, 0x78, -5, anchor=0), pats=pats)             # in front of the match: byte 1
    assert row(p, bt(1, EQ, 0x78, -6, anchor=0), pats=pats)             # byte 0
    assert not row(p, bt(1, GE, 0, -7, anchor=0), pats=pats)            # in front of the payload
    assert not row(b"xxLEN", bt(1, GE, 0, -1, anchor=0), pats=pats)     # no match, no field


def test_relative_is_existential_over_all_matches():
    pats = [b"LEN:"]
    p = b"LEN:\x01\x01 LEN:\x09\x09"
    assert row(p, bt(2, GT, 0x0800, 0, anchor=0), pats=pats)            # the first match fails (0x0101), the second serves
    assert row(p, bt(2, EQ, 0x0101, 0, anchor=0), pats=pats)
    assert not row(p, bt(2, EQ, 0x0505, 0, anchor=0), pats=pats)
    # a window on the anchor that leaves only the first match: the serving one is no match any more
    assert not row(p, bt(2, GT, 0x0800, 0, anchor=0), pats=pats, windows=[(0, 0)])
    assert row(p, bt(2, GT, 0x0800, 0, anchor=0), pats=pats, windows=[(1, None)])
    # overlapping starts: "aa" in "aaa\x05" starts at 0 and 1; only the second is followed by 0x05
    assert row(b"aaa\x05", bt(1, EQ, 5, 0, anchor=0), pats=[b"aa"])


def test_nocase_anchor_reads_the_original_bytes():
    pats, p = [b"len:"], b"LeN:AB"
    assert row(p, bt(2, EQ, 0x4142, 0, anchor=0), pats=pats, nocase=[True])
    assert not row(p, bt(2, EQ, 0x6162, 0, anchor=0), pats=pats, nocase=[True])     # not the folded copy's "ab"
    assert not row(p, bt(2, EQ, 0x4142, 0, anchor=0), pats=pats, nocase=[False])    # case-sensitive: no match of the anchor


def test_dns_capture():
    """very_big_udp.pcap is DNS: "is the QR bit set", "is QDCOUNT 1" split it, and every message is longer than its 12-byte header"""
    pays, _ = HM.capture(HM.pcap_frames(os.path.join(DATA, "very_big_udp.pcap")), "udp")
    tests = [bt(2, NE, 0, 2, mask=0x8000), bt(2, EQ, 1, 4), BM.isdataat(11)]
    rows = BM.bytetest_rows(pays, [], tests, whole=True)
    n = len(pays)
    assert n > 100
    assert 0 < rows[0].sum() < n and 0 < rows[1].sum() < n, rows.sum(axis=1).tolist()
    # the bytes themselves, once more without the model
    qr = np.array([len(p) >= 4 and bool(p[2] & 0x80) for p in pays])
    assert np.array_equal(rows[0], qr)
    # under the strlen rule a DNS header (0x00 in the flags or the counts) ends the text early: QDCOUNT is out of reach nearly everywhere
    assert BM.bytetest_rows(pays, [], tests[1:2]).sum() < rows[1].sum()


@pytest.mark.parametrize("op", [EQ, NE, LT, GT, LE, GE])
def test_every_operator_against_python(op):
    import operator
    fn = [operator.eq, operator.ne, operator.lt, operator.gt, operator.le, operator.ge][op]
    for a in (0, 1, 0x7F, 0x80, 0xFF):
        for v in (0, 1, 0x7F, 0x80, 0xFF, 0x100):
            assert row(bytes([a]), bt(1, op, v, 0), whole=True) == fn(a, v), (a, v)
