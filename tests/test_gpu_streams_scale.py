"""kmpgpu_load_streams past the grid sizes of its kernels, and on a source whose slots lie on both sides of byte 2^32.  Every comparison
is exact.  The model's Python loops are kept away from the large inputs: the records and the map come from stream_model.records_np (which
tests/test_stream_model.py holds to the loop model), and the expected arena is laid out by numpy from the source's bytes.

The caps, read off csrc/kmp_streams.hip:
  per-payload and per-stream kernels (heads, records, index): grid-stride, at most 1 024 blocks of 256 -- a second round from 262 145
      elements on.  N_BIG = 300 000 payloads are past it; so is the sort's single-block path.
  the scans: one tile of 1 024 sorted positions per block, the totals kernel 256 tiles per round -- 300 000 positions are 293 tiles, two
      rounds; the stream of 70 000 members crosses 68 tiles, so its positions are sums over many tiles minus the value at its head.
  the gather: at most 2 048 blocks of 4 wavefronts, each wavefront one contiguous span of whole rounds of 64 units (1 KiB): up to
      8 192 x 1 KiB = 8 MiB every wavefront has one round; the arena of test_one_long_stream is above 9 MiB, so wavefronts carry their
      place in the piece array from one round into the next.
  destination offsets as 64-bit values, > 4 GiB, and the high words of kmpgpu_stream.bytes and kmpgpu_stream_pos.pos:
      tests/test_gpu_high_destinations.py::test_streams_past_2_32 and test_stream_longer_than_2_32 (a stream of exactly 2^30 bytes).

Run on a real MI355X:  python -m pytest tests/test_gpu_streams_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import (B32, attach_placed, big_buffer, gm, meta_of_flows, placed_base, reset)  # noqa: E402,F401  (torch first; fixtures)

import seam_model as SM  # noqa: E402
import stream_model as TM  # noqa: E402
from multithreading_string_matching_amd.matcher import OPT_NONTEMPORAL, GpuMatcher  # noqa: E402
from test_gpu_streams import check_streams  # noqa: E402

N_BIG = 300_000
INDEX_ROUND = 1024 * 256
GATHER_ROUND = 2048 * 4 * 64 * 16
assert N_BIG > INDEX_ROUND


@pytest.fixture(scope="module")
def sm():
    m = GpuMatcher(0)
    yield m
    m.close()


def random_arena(rng, lens):
    """a packed arena of random non-zero bytes with 0x00 behind every payload's end"""
    lens = np.asarray(lens, dtype=np.uint32)
    size = np.maximum(16, (lens.astype(np.uint64) + 15) // 16 * 16)
    off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64)
    arena = rng.integers(1, 256, int(size.sum()) + 64, dtype=np.uint8)
    mask = np.ones(len(arena), dtype=bool)
    L = lens.astype(np.int64)
    idx = np.repeat(off.astype(np.int64), L) + (np.arange(int(L.sum())) - np.repeat(np.cumsum(L) - L, L))
    mask[idx] = False
    arena[mask] = 0
    return arena, off, lens


def expected_arena(arena, off, lens, recs, pos):
    """(bytes, off, len) of the packed streams, from the source's bytes by numpy"""
    slen = recs["len"].astype(np.int64)
    size = np.maximum(16, (slen + 15) // 16 * 16)
    soff = np.concatenate([[0], np.cumsum(size)[:-1]])
    want = np.zeros(int(size.sum()), dtype=np.uint8)
    L = lens.astype(np.int64)
    st, at = pos["stream"].astype(np.int64), pos["pos"].astype(np.int64)
    take = np.clip(slen[st] - at, 0, L)                        # bytes of every member in front of the cut
    j = np.arange(int(take.sum())) - np.repeat(np.cumsum(take) - take, take)
    want[np.repeat(soff[st] + at, take) + j] = arena[np.repeat(off.astype(np.int64), take) + j]
    return want, soff.astype(np.uint64), slen.astype(np.uint32)


def check_big(dst, arena, off, lens, meta, depth, directed=False):
    recs, pos = TM.records_np(meta, lens, depth, directed)
    got, gmap = dst.streams(), dst.stream_map()
    assert got.tobytes() == recs.tobytes(), np.flatnonzero(got != recs)[:4]
    assert gmap.tobytes() == pos.tobytes(), np.flatnonzero(gmap != pos)[:4]
    want, soff, slen = expected_arena(arena, off, lens, recs, pos)
    a, o, l = dst.arena_download()
    assert np.array_equal(o, soff) and np.array_equal(l, slen)
    assert not a[len(want):].any()
    bad = np.flatnonzero(a[:len(want)] != want)
    assert bad.size == 0, [(int(b), int(np.searchsorted(soff, b, side="right")) - 1) for b in bad[:8]]
    assert dst.meta().tobytes() == meta[recs["first_packet"].astype(np.int64)].tobytes()
    return recs, pos


@pytest.mark.parametrize("nontemporal", [1, 0])
def test_many_small_payloads(gm, sm, nontemporal):
    """300 000 payloads of 0 .. 40 bytes in about 3 000 flows: every per-payload kernel has a second round, the scans two rounds of tiles"""
    rng = np.random.default_rng(77)
    arena, off, lens = random_arena(rng, rng.integers(0, 41, N_BIG))
    k = np.arange(N_BIG)
    meta = meta_of_flows((k * 2654435761 >> 7) % 3000, seed=4)
    reset(gm, sm)
    try:
        sm.set_option(OPT_NONTEMPORAL, nontemporal)
        gm.set_patterns([b"\x41\x42"])
        gm.load_arena(arena, off, lens)
        gm.set_meta(meta)
        n_flows = gm.build_flows()
        for depth in (1 << 30, 1000):
            n = sm.load_streams(gm, depth)
            recs, pos = check_big(sm, arena, off, lens, meta, depth)
            assert n == len(recs) == N_BIG - len(SM.records_np(meta, lens, 98)) and 3000 <= n <= 6000
            assert (recs["bytes"] > recs["len"]).any() == (depth == 1000)
        assert sm.build_flows() == n_flows and sm.flow_ids().tolist() == recs["flow"].tolist()
    finally:
        reset(gm, sm)


def test_every_payload_a_stream(gm, sm):
    """300 000 streams: the per-stream kernels and the slot scan past their first round"""
    rng = np.random.default_rng(78)
    arena, off, lens = random_arena(rng, rng.integers(0, 41, N_BIG))
    meta = meta_of_flows(np.arange(N_BIG), seed=4)
    reset(gm, sm)
    gm.set_patterns([b"\x41\x42"])
    gm.load_arena(arena, off, lens)
    gm.set_meta(meta)
    assert gm.build_flows() == N_BIG
    assert sm.load_streams(gm, 24) == N_BIG
    check_big(sm, arena, off, lens, meta, 24)


def test_one_long_stream(gm, sm):
    """one stream of 70 000 members with a cut inside it: the segmented sum crosses 68 scan tiles, the arena is past the gather's cap"""
    rng = np.random.default_rng(79)
    n = 70_000
    arena, off, lens = random_arena(rng, rng.integers(100, 201, n))
    lens_in = lens.copy()
    meta = meta_of_flows(np.zeros(n, dtype=np.int64), seed=4)
    meta[:] = meta[0]                                           # one direction
    total = int(lens_in.sum())
    depth = total - 500_000
    assert depth > GATHER_ROUND + (1 << 20)
    reset(gm, sm)
    gm.set_patterns([b"\x41\x42"])
    gm.load_arena(arena, off, lens)
    gm.set_meta(meta)
    assert gm.build_flows() == 1
    assert sm.load_streams(gm, depth) == 1
    recs, pos = check_big(sm, arena, off, lens, meta, depth)
    assert recs["len"].tolist() == [depth] and recs["bytes"].tolist() == [total] and recs["n_packets"].tolist() == [n]
    assert int(pos["pos"][-1]) == total - int(lens_in[-1])


def test_source_on_both_sides_of_2_32(gm, sm, big_buffer):
    """the source attached with slots in front of, across and behind byte 2^32 of one buffer: the pieces' source addresses are 64-bit"""
    rng = np.random.default_rng(80)
    n = 300
    lens = rng.choice([0, 1, 5, 16, 17, 33, 200, 700], n)
    lens[100] = 200
    pay = [bytes(rng.integers(1, 256, int(x), dtype=np.uint8)) for x in lens]
    slots = [t + b"\xAA" * (TM.slot(len(t)) - len(t)) for t in pay]          # dirty padding: nothing behind a member's end is copied
    meta = meta_of_flows(rng.integers(0, 12, n), seed=5)
    base = placed_base("split", pay, slots, k=100)
    reset(gm, sm)
    gm.set_patterns([b"x"])
    keep = attach_placed(gm, pay, slots, base, big_buffer)
    gm.set_meta(meta)
    gm.build_flows()
    assert base < B32 < base + sum(len(s) for s in slots)
    for depth in (1 << 30, 3000):
        sm.load_streams(gm, depth)
        streams, recs, pos = check_streams(sm, pay, meta, depth)
        assert len(streams) > 12 and any(int(r["first_packet"]) < 100 < int(r["last_packet"]) for r in recs)      # streams with members on both sides
    del keep
