"""tests/link_model.py held to hand-written cases: the three map kinds, bits at and above n_dst, and an index map with NONE, with an
index at and above n_src, and many payloads on one source payload.  No device needed."""
import numpy as np
import pytest

import link_model as LM


def bits(s):
    return np.array([ch == "1" for ch in s], dtype=bool)


def test_same_is_the_identity():
    rows = np.array([bits("10110"), bits("00001")])
    assert np.array_equal(LM.link(rows, 5, 5, LM.SAME), rows)
    with pytest.raises(ValueError):
        LM.link(rows, 5, 6, LM.SAME)


def test_bitmap_takes_the_jth_set_bit():
    # dst holds 7 payloads; 1, 2, 5 are the source's payloads 0, 1, 2
    rows = np.array([bits("101"), bits("010"), bits("000")])
    got = LM.link(rows, 3, 7, LM.BITMAP, bits("0110010"))
    assert got.astype(int).tolist() == [[0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0, 0], [0] * 7]


def test_bitmap_words_and_bools_agree():
    words = np.array([0b0100110], dtype=np.uint64)
    rows = np.array([bits("101")])
    assert np.array_equal(LM.link(rows, 3, 7, LM.BITMAP, words), LM.link(rows, 3, 7, LM.BITMAP, bits("0110010")))


def test_bitmap_ignores_bits_at_and_above_n_dst():
    # n_dst = 4: bits 4 .. 63 of the word are garbage and name no payload
    rows = np.array([bits("11")])
    clean = np.array([0b0101], dtype=np.uint64)
    dirty = clean | np.uint64(0xFFFFFFFFFFFFFFF0)
    want = [[1, 0, 1, 0]]
    assert LM.link(rows, 2, 4, LM.BITMAP, clean).astype(int).tolist() == want
    assert LM.link(rows, 2, 4, LM.BITMAP, dirty).astype(int).tolist() == want
    assert LM.link(rows, 2, 4, LM.BITMAP, dirty).shape == (1, 4)


def test_bitmap_popcount_must_be_n_src():
    rows = np.array([bits("11")])
    with pytest.raises(ValueError):
        LM.link(rows, 2, 4, LM.BITMAP, np.array([0b0111], dtype=np.uint64))
    with pytest.raises(ValueError):
        LM.link(rows, 2, 4, LM.BITMAP, np.array([0b0001], dtype=np.uint64))
    # ... counted below n_dst only
    with pytest.raises(ValueError):
        LM.link(rows, 2, 4, LM.BITMAP, np.array([0b10001], dtype=np.uint64))


def test_bitmap_all_zero_and_all_ones():
    assert not LM.link(np.zeros((2, 0), bool), 0, 5, LM.BITMAP, np.zeros(1, np.uint64)).any()
    rows = np.array([bits("10011")])
    assert np.array_equal(LM.link(rows, 5, 5, LM.BITMAP, np.array([0b11111], np.uint64)), rows)


def test_index_none_out_of_range_and_many_to_one():
    rows = np.array([bits("10"), bits("01")])
    idx = np.array([0, 0, 1, LM.NONE, 2, 1, 0], dtype=np.uint32)       # 2 == n_src: none, as NONE
    got = LM.link(rows, 2, 7, LM.INDEX, idx)
    assert got.astype(int).tolist() == [[1, 1, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 1, 0]]
    with pytest.raises(ValueError):
        LM.link(rows, 2, 7, LM.INDEX, idx[:6])
    with pytest.raises(ValueError):
        LM.link(rows, 2, 7, LM.INDEX, idx.astype(np.int64))


def test_index_with_an_empty_source():
    got = LM.link(np.zeros((3, 0), bool), 0, 4, LM.INDEX, np.array([0, 1, LM.NONE, 0], dtype=np.uint32))
    assert got.shape == (3, 4) and not got.any()


def test_links_chain():
    # decoded (2 payloads, the changed ones of 4) -> raw_uri (4 payloads, the present ones of 6) -> capture (6 payloads)
    verdict = np.array([bits("01")])
    mid = LM.link(verdict, 2, 4, LM.BITMAP, bits("0101"))
    assert mid.astype(int).tolist() == [[0, 0, 0, 1]]
    top = LM.link(mid, 4, 6, LM.BITMAP, bits("110110"))
    assert top.astype(int).tolist() == [[0, 0, 0, 0, 1, 0]]
