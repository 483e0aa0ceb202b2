"""kmpgpu_load_streams_ordered past the grid sizes of its kernels, and on a source whose slots lie on both sides of byte 2^32.  Every
comparison is exact.  The model's Python loops are kept away from the large inputs: the capture is PERIODIC -- period r repeats period 0's
payloads, directions and sequence numbers between flows of its own --, so its streams, records and arena are period 0's, which
tests/stream_seq_model.py builds, repeated with the indices moved on; the totals follow in closed form.

The caps, read off csrc/kmp_streams_seq.hip:
  per-payload and per-stream kernels (heads, keys, records, index): grid-stride, at most 1 024 blocks of 256 -- a second round from
      262 145 elements on.  test_many_small_payloads has 262 144 + 1 000 payloads, test_many_streams more than 262 144 streams.
  the scans: one tile of 1 024 ordered positions per block, the two totals kernels 256 tiles per round -- 263 144 positions are 257 tiles,
      two rounds; a stream of several thousand members crosses tiles, so its maximum and its sums are carried across them.
  the source's addresses as 64-bit values: test_source_on_both_sides_of_2_32, the way tests/test_gpu_streams_scale.py reaches it.

Run on a real MI355X:  python -m pytest tests/test_gpu_streams_seq_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import (B32, FLOW_B, attach_placed, big_buffer, gm, load, meta_of_flows, placed_base, reset)  # noqa: E402,F401  (torch first; fixtures)

import stream_model as TM  # noqa: E402
import stream_seq_model as QM  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402
from test_gpu_streams_seq import FULL, _spread, check  # noqa: E402

INDEX_ROUND = 1024 * 256


@pytest.fixture(scope="module")
def sm():
    m = GpuMatcher(0)
    yield m
    m.close()


def periodic(pay, meta, seq, reps):
    """the capture repeated `reps` times, period r between flows of its own (the address that is not FLOW_B moved on by r << 16)"""
    P = len(pay)
    r = np.repeat(np.arange(reps, dtype=np.uint32), P) << np.uint32(16)
    big = np.tile(meta, reps)
    for field in ("src_ip", "dst_ip"):
        big[field] = np.where(big[field] == FLOW_B, big[field], big[field] + r)
    return pay * reps, big, np.tile(seq, reps)


def check_periodic(dst, model, meta, P, reps, depth):
    """dst against period 0's model repeated: records and map with their indices moved on, segs, orders, index and arena tiled"""
    streams, recs, pos, segs, orders, _ = model
    S, F = len(recs), int(recs["flow"].max()) + 1
    recs = recs.copy()
    recs["len"] = np.minimum(recs["bytes"], depth)
    want_recs, want_pos = np.tile(recs, reps), np.tile(pos, reps)
    rs, rp = np.repeat(np.arange(reps), S), np.repeat(np.arange(reps), P)
    want_recs["first_packet"] += (rs * P).astype(np.uint64)
    want_recs["last_packet"] += (rs * P).astype(np.uint64)
    want_recs["flow"] += (rs * F).astype(np.uint32)
    want_pos["stream"] += (rp * S).astype(np.uint32)
    got, gmap = dst.streams(), dst.stream_map()
    assert got.tobytes() == want_recs.tobytes(), np.flatnonzero(got != want_recs)[:4]
    assert gmap.tobytes() == want_pos.tobytes(), np.flatnonzero(gmap != want_pos)[:4]
    gsegs, gorders = dst.stream_segs(), dst.stream_orders()
    assert gsegs.tobytes() == np.tile(segs, reps).tobytes(), np.flatnonzero(gsegs != np.tile(segs, reps))[:4]
    assert gorders.tobytes() == np.tile(orders, reps).tobytes(), np.flatnonzero(gorders != np.tile(orders, reps))[:4]
    per, poff, pln = TM.arena([s[:depth] for s in streams])
    a, o, l = dst.arena_download()
    assert np.array_equal(l, np.tile(pln, reps))
    assert np.array_equal(o, (np.tile(poff, reps) + np.repeat(np.arange(reps, dtype=np.uint64), S) * np.uint64(len(per))))
    assert len(a) >= reps * len(per) and not a[reps * len(per):].any()
    body = a[:reps * len(per)].reshape(reps, len(per))
    bad = np.argwhere(body != per)
    assert bad.size == 0, bad[:8].tolist()
    assert dst.meta().tobytes() == meta[want_recs["first_packet"].astype(np.int64)].tobytes()
    # closed form
    assert dst.arena_info() == (reps * S, reps * int(recs["len"].sum()))
    assert int(gorders["dup_bytes"].sum()) == reps * int(orders["dup_bytes"].sum()) and int(gsegs["take"].sum()) == reps * int(recs["bytes"].sum())
    assert int(gorders["n_gaps"].sum()) == reps * int(orders["n_gaps"].sum())


def _run(gm, sm, P, n_flows, lengths, reps, depths, seed):
    rng = np.random.default_rng(seed)
    flow = np.concatenate([np.arange(n_flows), rng.integers(0, n_flows, P - n_flows)])
    meta = meta_of_flows(flow, seed=seed)
    meta["proto"] = np.where(flow % 5 == 0, 17, 6)
    pay, seq = _spread(rng, meta, lengths)
    model = QM.build(pay, meta, seq, FULL)
    big_pay, big_meta, big_seq = periodic(pay, meta, seq, reps)
    reset(gm, sm)
    gm.set_patterns([b"\x41\x42"])
    load(gm, big_pay)
    gm.set_meta(big_meta)
    assert gm.build_flows() == reps * n_flows
    for depth in depths:
        assert sm.load_streams(gm, depth, seq=big_seq) == reps * len(model[1])
        check_periodic(sm, model, big_meta, P, reps, depth)
    return model


def test_many_small_payloads(gm, sm):
    """262 144 + 1 000 payloads of 0 .. 3 bytes, 8 periods of 32 893 in 16 flows each: every per-payload kernel has a second round, the
    scans two rounds of tiles, and streams of more than a thousand members, many of them covered or empty, cross the tiles"""
    P, reps = (INDEX_ROUND + 1000) // 8, 8
    assert P * reps == INDEX_ROUND + 1000
    model = _run(gm, sm, P, 16, np.arange(0, 4), reps, (FULL, 100), seed=31)
    assert model[1]["n_packets"].max() > 1024 and (model[1]["bytes"] > 100).any()


def test_many_streams(gm, sm):
    """more than 262 144 streams: the per-stream kernels and the slot scan past their first round"""
    P, n_flows, reps = 1500, 800, 330                           # at least one stream per flow: 264 000 and more
    model = _run(gm, sm, P, n_flows, np.arange(0, 20), reps, (24,), seed=32)
    assert reps * len(model[1]) > INDEX_ROUND


def test_source_on_both_sides_of_2_32(gm, sm, big_buffer):
    """the source attached with slots in front of, across and behind byte 2^32 of one buffer: the pieces' source addresses are 64-bit, and
    the fetch starts `skip` bytes inside a member on either side"""
    rng = np.random.default_rng(33)
    n = 300
    flow = np.concatenate([np.arange(12), rng.integers(0, 12, n - 12)])
    meta = meta_of_flows(flow, seed=5)
    meta["proto"] = 6
    pay, seq = _spread(rng, meta, np.array([0, 1, 5, 16, 17, 33, 200, 700]))
    pay[100] = bytes(rng.integers(1, 256, 200, dtype=np.uint8))
    slots = [t + b"\xAA" * (TM.slot(len(t)) - len(t)) for t in pay]          # dirty padding: nothing behind a member's end is copied
    model = QM.build(pay, meta, seq, FULL)
    assert model[3]["take"][100] > 0
    base = placed_base("split", pay, slots, k=100)
    reset(gm, sm)
    gm.set_patterns([b"x"])
    keep = attach_placed(gm, pay, slots, base, big_buffer)
    gm.set_meta(meta)
    gm.build_flows()
    assert base < B32 < base + sum(len(s) for s in slots)
    for depth in (FULL, 3000):
        sm.load_streams(gm, depth, seq=seq)
        streams, recs = check(sm, model, meta, depth)
        assert len(streams) > 12 and any(int(r["first_packet"]) < 100 < int(r["last_packet"]) for r in recs)
    del keep
