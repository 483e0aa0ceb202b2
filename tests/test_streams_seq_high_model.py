"""The expectations of tests/test_gpu_streams_seq_high.py against tests/stream_seq_model.py's build, on inputs small enough to build
everything in full: three periods and a rest.  No GPU: what lays the capture out on the device runs with torch on the CPU.

  stream_seq_model.build_np (lexsort, running maximum)    build, on the schedule with short payloads, on the periodic capture and on the
                                                          20 000 random small streams of tests/test_stream_seq_model.py as one capture
  tiled (one period's model moved on)                     build of the whole capture: records, map, segs, orders, index, arena, tag counts
  schedule, scheduled_tallies, scheduled_locate,          build of 2 570 + 430 payloads on the schedule
  kept_period
  capture_meta, capture_seq, periodic_source              the listed capture and decode_model.packed_image of it
"""
import numpy as np
import pytest

from gpu_support import PERIOD, check_periodic_bytes, meta_of_flows, periodic_source, tagged

import decode_model as DM
import stream_model as TM
import stream_seq_model as QM
import test_gpu_high_destinations as HD
import test_gpu_streams_seq_high as SH
from header_model import META_DTYPE

REPS = 3
FULL = 1 << 30


def same(got, want):
    for a, b, name in zip(got, want, ("recs", "pos", "segs", "orders")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, np.flatnonzero(a != b)[:4])


@pytest.fixture(scope="module")
def capture():
    """(the period, its model, the rest's model, the whole capture listed and its model)"""
    pay, meta, seq = SH.ordered_period()
    big_pay = pay * REPS + pay[:HD.REST]
    big_meta = SH.capture_meta(meta, REPS, HD.REST)
    big_seq = np.concatenate([np.tile(seq, REPS), seq[:HD.REST]])
    return ((pay, meta, seq), QM.build(pay, meta, seq, FULL), QM.build(pay[:HD.REST], meta[:HD.REST], seq[:HD.REST], FULL),
            (big_pay, big_meta, big_seq), QM.build(big_pay, big_meta, big_seq, FULL))


def test_the_period_is_what_the_test_needs(capture):
    (pay, meta, seq), model, rest, _, _ = capture
    recs, segs, orders = model[1], model[3], model[4]
    assert len(recs) == len(rest[1]) == 2 * SH.PERIOD_FLOWS and (orders["tcp"] == 0).sum() == 2 and seq.all()
    assert ((segs["skip"] > 0) & (segs["take"] > 0)).sum() > 15 and ((segs["take"] == 0) & (segs["skip"] > 0)).sum() > 10
    assert orders["n_gaps"].sum() > 5 and orders["dup_bytes"].sum() > 3000
    assert meta[:SH.PERIOD_FLOWS].tobytes() != meta[1:SH.PERIOD_FLOWS + 1].tobytes()
    assert (orders["seq_base"][orders["tcp"] == 1] >= (1 << 32) - 500).sum() >= 2          # streams that wrap


@pytest.mark.parametrize("depth", ["full", "cut", 17, 1])
def test_tiled_is_the_model_of_the_whole_capture(capture, depth):
    (pay, meta, seq), model, rest, (big_pay, big_meta, big_seq), whole = capture
    depth = {"full": FULL, "cut": SH.forward_cut(model)}.get(depth, depth)
    want = SH.tiled(model, rest, PERIOD, REPS, depth)
    streams = [s[:depth] for s in whole[0]]
    same((want["recs"], want["pos"], want["segs"], want["orders"]), (HD.cut_to(whole[1], depth), whole[2], whole[3], whole[4]))
    arena, off, ln = TM.arena(streams)
    assert np.array_equal(want["off"], off) and np.array_equal(want["len"], ln) and want["end"] == len(arena)
    assert np.array_equal(np.concatenate([np.tile(want["per"], REPS), want["head"]]), arena)
    check_periodic_bytes(np.concatenate([arena, np.zeros(64, np.uint8)]), want, rows=2)
    assert want["tags"].tolist() == [sum(s.split(b"\0")[0].count(tag) for s in streams) for tag in HD.TAGS]
    assert want["n_flows"] == int(whole[1]["flow"].max()) + 1
    if depth == FULL:                                               # a tag inside a covered front does not count
        assert want["tags"].sum() < len(big_pay) - (whole[3]["take"] == 0).sum() and (want["tags"] >= REPS).sum() > 200
    # the numpy formulation on the same capture
    same(QM.build_np([len(t) for t in big_pay], big_meta, big_seq, depth), (HD.cut_to(whole[1], depth), whole[2], whole[3], whole[4]))


def test_a_wrong_byte_is_found(capture):
    _, model, rest, _, _ = capture
    want = SH.tiled(model, rest, PERIOD, REPS, FULL)
    a = np.concatenate([np.tile(want["per"], REPS), want["head"], np.zeros(64, np.uint8)])
    for at in (0, len(want["per"]) + 5, 2 * len(want["per"]) + 1, want["end"] - 1, want["end"], want["end"] + 63):
        b = a.copy()
        b[at] ^= 1
        with pytest.raises(AssertionError):
            check_periodic_bytes(b, want, rows=2)


def test_the_device_layout_is_the_listed_capture(capture):
    (pay, meta, seq), _, _, (big_pay, big_meta, big_seq), _ = capture
    n = len(big_pay)
    d_seq = SH.capture_seq(seq, REPS, HD.REST, device="cpu")
    assert d_seq.is_contiguous() and d_seq.element_size() == 4 and np.array_equal(d_seq.numpy().view(np.uint32), big_seq)
    arena, off, ln = DM.packed_image(big_pay)
    d_arena, d_off, d_len = periodic_source(pay, n, device="cpu")
    assert np.array_equal(d_off.numpy(), off.astype(np.int64)) and np.array_equal(d_len.numpy(), ln.astype(np.int32))
    assert np.array_equal(d_arena.numpy()[:len(arena)], arena) and not d_arena.numpy()[len(arena):].any()
    # period r lies between flows of its own, numbered in the order of the period's
    fo = TM.members(big_meta)
    assert len(fo) == (REPS + 1) * 2 * SH.PERIOD_FLOWS
    assert [f for f, d, ks in fo if d == 0] == list(range((REPS + 1) * SH.PERIOD_FLOWS))
    assert all(ks[0] // PERIOD == f // SH.PERIOD_FLOWS == ks[-1] // PERIOD for f, d, ks in fo)


# ------------------------------------------------------------------------------------------------
# the schedule
# ------------------------------------------------------------------------------------------------
def short_period(L=120):
    rng = np.random.default_rng(7)
    return [tagged(HD.filler(rng, L), e) for e in range(PERIOD)]


def one_flow(n):
    meta = np.repeat(meta_of_flows(np.zeros(1, dtype=np.int64), seed=4), n)
    meta["proto"] = 6
    return meta


def test_the_schedule_against_the_model():
    L, n = 120, PERIOD * SH.GROUP + 430
    pay = short_period(L)
    listed = [pay[k % PERIOD] for k in range(n)]
    meta, seq = one_flow(n), SH.scheduled_seq(n, L)
    streams, recs, pos, segs, orders, origin = QM.build(listed, meta, seq, FULL)
    assert len(streams) == 1 and int(seq[0]) == SH.ISN and int(seq[-1]) < SH.ISN
    for depth in (FULL, 200_001, 16, 1):
        same(QM.build_np([L] * n, meta, seq, depth), (HD.cut_to(recs, depth), pos, segs, orders))
    # the schedule is what it says
    g = 5 * SH.GROUP
    assert segs["take"][g + 4] == 0 and segs["skip"][g + 4] == L and segs["seq_off"][g + 4] == segs["seq_off"][g + 3]
    assert segs["skip"][g + 7] == 100 and segs["take"][g + 7] == L - 100 and pos["pos"][g + 9] < pos["pos"][g + 8]
    assert segs["seq_off"][g] - (segs["seq_off"][g - 2] + L) == 3 and not segs["skip"][np.arange(n) % SH.GROUP < 4].any()
    # closed forms
    o = orders[0]
    assert (int(recs["bytes"][0]), int(o["n_gaps"]), int(o["gap_bytes"]), int(o["dup_bytes"])) == SH.scheduled_tallies(n, L)
    assert int(o["seq_base"]) == SH.ISN and int(o["tcp"]) == 1
    for x in list(range(0, 3 * (9 * L - 100))) + [len(streams[0]) - 1, 123_457]:
        assert SH.scheduled_locate(x, L) == origin[0][x], x
    # one period of kept bytes, and the stream as its repetition
    whole = SH.kept_period(pay, segs, pos, PERIOD * SH.GROUP)
    data = np.frombuffer(streams[0], dtype=np.uint8)
    assert len(whole) == PERIOD * (9 * L - 100) == int(pos["pos"][PERIOD * SH.GROUP])
    assert np.array_equal(data[:len(whole)], whole) and np.array_equal(data[len(whole):], whole[:len(data) - len(whole)])


def test_the_numpy_formulation_on_random_small_streams():
    """the 20 000 streams of tests/test_stream_seq_model.py::test_the_two_formulations_agree_on_random_streams, as the flows of one capture
    (every tenth one UDP), captured interleaved"""
    rng = np.random.default_rng(1)
    rows, pay, seq = [], [], []
    for f in range(20000):
        m = int(rng.integers(1, 7))
        lens = rng.integers(0, 6, m)
        start = int(rng.choice([0, 1000, 0xFFFFFFF8, 0x7FFFFFFC]))
        for x, q in zip(lens, (start + rng.integers(0, 12, m)) & 0xFFFFFFFF):
            rows.append(f)
            pay.append(bytes(rng.integers(1, 256, int(x), dtype=np.uint8)))
            seq.append(int(q))
    order = rng.permutation(len(rows))
    flow = np.array(rows)[order]
    meta = np.zeros(len(flow), dtype=META_DTYPE)
    meta["src_ip"], meta["dst_ip"], meta["src_port"], meta["dst_port"] = 0x0A000001 + flow, 0xC0A80101, 1000, 80
    meta["proto"] = np.where(flow % 10 == 9, 17, 6)
    back = rng.random(len(flow)) < 0.3
    meta["src_ip"][back], meta["dst_ip"][back] = meta["dst_ip"][back], meta["src_ip"][back]
    meta["src_port"][back], meta["dst_port"][back] = 80, 1000
    pay, seq = [pay[i] for i in order], np.array(seq, dtype=np.uint32)[order]
    streams, recs, pos, segs, orders, _ = QM.build(pay, meta, seq, 9)
    assert len(recs) > 25000 and (recs["bytes"] > recs["len"]).any() and orders["n_gaps"].sum() > 1000 and orders["dup_bytes"].sum() > 10000
    same(QM.build_np([len(t) for t in pay], meta, seq, 9), (recs, pos, segs, orders))
