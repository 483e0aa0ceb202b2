"""kmpgpu_load_streams_ordered on small data in WIDE sequence space: streams whose members span up to the 2^31 - 1 of sequence space that
include/kmpgpu.h promises to order correctly.  tests/test_gpu_streams_seq.py and tests/test_gpu_streams_seq_scale.py draw every stream's
offsets from a few KB with holes of 1 to 30 bytes, so rel + 2^31 differed in its low 16 bits or so (the upper digit passes of the second
sort were trivial) and off, end = off + L, the running maximum M, the signed ahead = M - off, gap_bytes and min rel all stayed tiny.  Here
the same kind of stream (_segments: duplicates, partial overlaps, empty members, small holes) is STRETCHED: at up to 8 cut points among its
distinct starts every start at or behind the cut moves on by a hole, the holes sized so that max(off + L) - min off is 2^31 - 1 for half of
the streams and a random value in [2^24, 2^31) for the others.  What lies between two cuts keeps its duplicates and overlaps.  The members
go out in a random order under a random ISN (every third stream's within 500 of 2^32, so the wide span wraps as well), which puts the
first captured member -- the one rel is measured against -- anywhere in the span.

The expectation is tests/stream_seq_model.py's build (a dict of cells per stream; no running maximum, no sort key) through
test_gpu_streams_seq.check: records, map, segs, orders, index, every arena byte and the metadata, exactly.  The input is asserted on the
model before the GPU sees it (gap_bytes, seq_off and min rel near their bounds, enough partly and fully covered members).

test_one_stream_across_scan_tiles: kmp_sseq_max_scan_kernel carries a maximum near 2^31 through blk_mx over four tiles.  A payload is at
most a few hundred bytes here, so the stream's lowest member cannot itself end near 2^31: the stream opens with one member at offset 0,
and the FIRST member of the top run, at 2^31 - 217, ends at 2^31 - 1 - 16 with 3 300 members inside it -- every one fully covered, a
0-byte piece in the middle of the stream -- and one member across its end.  The reverse: one member at offset 0 and 3 300 one-byte members
under 2^31, one free sequence offset in front of each, every one opening a gap.

Run on a real MI355X:  python -m pytest tests/test_gpu_streams_seq_span.py -m gpu
Measured there (one process, call time): the first case 0.19 s with the context's set-up, test_one_stream_across_scan_tiles 0.10 s, every
other case 0.01 s or less; the module 2.5 s.

Checked to bite, on memory-safe scratch builds that were never committed (tests/test_gpu_streams_seq_high.py lists all of them):
  5   kmp_sseq_take_scan_kernel, `ahead` computed as (int32_t)((uint32_t)to - M.off): this module PASSES, and so does every other one --
      the change is no fault.  Members are visited in ascending off, so to - off <= the longest member (2^30); and the first captured
      member has rel = 0, so two members next to each other in the order lie at most 2^31 apart, and off - to <= 2^31.  Every value of
      `ahead` lies in [-2^31, 2^30] and survives the 32-bit difference, for every input, not only those inside the promise.  The issue
      that asked for this module named the build as one that must fail here; it cannot fail any correct test.
  5b  instead, the fault this module is there for: the running maximum packed as stream << 30 | end (kmp_sseq_max_scan_kernel,
      covered_to, SSEQ_END_MASK) -- too few bits for an end of 2^30 and more, self-consistent sums, no address involved.  All 10 tests of
      this module fail (records, segs and bytes differ from the first wide stream on); the 34 tests of tests/test_gpu_streams_seq.py and
      tests/test_gpu_streams_seq_scale.py pass on that build: the gap this module closes.
"""
import functools

import numpy as np
import pytest

from gpu_support import gm, load, meta_of_flows, reset, torch  # noqa: F401  (gm: the context fixture; torch first)

import match_model as MM
import stream_model as TM
import stream_seq_model as QM
from multithreading_string_matching_amd.matcher import OPT_NONTEMPORAL, GpuMatcher, stream_locate_ordered
from test_gpu_streams_seq import FULL, X, Z, _isn, _meta, _put, _segments, check

pytestmark = pytest.mark.gpu

BOUND = (1 << 31) - 1                      # the widest span the header allows: max(off + L) - min off


@pytest.fixture(scope="module")
def sm():
    """the second context: the one that owns the streams"""
    m = GpuMatcher(0)
    yield m
    m.close()


def stretch(rng, segs, span, cuts=8):
    """the segments [(offset, bytes)] with every start at or behind up to `cuts` random cut points (distinct starts, not the lowest) moved
    on by a hole, the holes summing to what brings max(off + L) - min off to `span`"""
    starts = sorted({o for o, _ in segs})
    have = max(o + len(b) for o, b in segs) - starts[0]
    if len(starts) < 2 or span <= have:
        return segs
    at = sorted(rng.choice(starts[1:], size=min(cuts, len(starts) - 1), replace=False).tolist())
    need = span - have
    marks = np.sort(rng.integers(0, need + 1, len(at) - 1))
    holes = np.diff(np.concatenate([[0], marks, [need]])).tolist()
    assert sum(holes) == need
    return [(o + sum(h for c, h in zip(at, holes) if o >= c), b) for o, b in segs]


def spread_wide(rng, meta, lengths):
    """test_gpu_streams_seq._spread with every TCP stream stretched: every other one to the bound, the others to a random span"""
    pay, seq = [b""] * len(meta), np.zeros(len(meta), dtype=np.uint32)
    spans = []
    for s, (f, d, ks) in enumerate(TM.members(meta)):
        isn = _isn(rng, s)
        span = BOUND if s % 2 == 0 else int(rng.integers(1 << 24, 1 << 31))
        segs = stretch(rng, _segments(rng, len(ks), lengths), span)
        spans.append(max(o + len(b) for o, b in segs) - min(o for o, _ in segs))
        for k, j in zip(ks, rng.permutation(len(ks))):
            pay[k], seq[k] = segs[j][1], (isn + segs[j][0]) & 0xFFFFFFFF
    return pay, seq, spans


def min_rel(meta, seq):
    """per stream: min over its members of int32(seq[k] - seq[first captured member])"""
    return [min(QM.rel(seq[k], seq[ks[0]]) for k in ks) for _, _, ks in TM.members(meta)]


@functools.lru_cache(maxsize=None)
def wide():
    """about 1 500 payloads of 0 .. 200 bytes in 12 flows, both directions, flows 0 and 6 UDP"""
    rng = np.random.default_rng(41)
    n, n_flows = 1500, 12
    flow = np.concatenate([np.arange(n_flows), rng.integers(0, n_flows, n - n_flows)])
    meta = meta_of_flows(flow, seed=41)
    meta["proto"] = np.where(flow % 6 == 0, 17, 6)
    pay, seq, spans = spread_wide(rng, meta, np.arange(0, 201))
    model = QM.build(pay, meta, seq, FULL)
    recs, segs, orders = model[1], model[3], model[4]
    tcp = orders["tcp"] == 1
    lens = np.array([len(t) for t in pay])
    # the case cannot silently degenerate
    assert 0 < (~tcp).sum() < len(tcp) and set(recs["dir"].tolist()) == {0, 1}
    assert sum(x == BOUND for x in spans) >= tcp.sum() // 2 - 1 and all(x < 1 << 31 for x in spans)
    assert orders["gap_bytes"].max() >= (1 << 31) - (1 << 16)
    assert segs["seq_off"].max() >= (1 << 31) - 256
    assert sum(r < -(1 << 30) for r in min_rel(meta, seq)) >= 4
    assert ((segs["skip"] > 0) & (segs["take"] > 0)).sum() > 50                  # partly covered
    assert ((segs["take"] == 0) & (lens > 0)).sum() > 200                        # fully covered
    assert (orders["seq_base"][tcp] >= (1 << 32) - 500).sum() >= 3               # wide spans that wrap
    return pay, meta, seq, model


CASES = [(1, "loaded", "host", 1), (17, "dirty", "device", 0), (4096, "in_place", "host", 0), (4096, "loaded", "device", 1),
         (FULL, "loaded", "host", 0), (FULL, "dirty", "device", 1), (FULL, "in_place", "device", 0)]


@pytest.mark.parametrize("depth, form, seq_on, nontemporal", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_wide_spans_against_the_model(gm, sm, depth, form, seq_on, nontemporal):
    pay, meta, seq, model = wide()
    reset(gm, sm)
    try:
        sm.set_option(OPT_NONTEMPORAL, nontemporal)
        gm.set_patterns([b"x"])
        keep = _put(gm, pay, meta, form)
        gm.build_flows()
        handed = torch.from_numpy(seq.view(np.int32)).cuda() if seq_on == "device" else seq
        assert sm.load_streams(gm, depth, seq=handed) == len(model[1])
        check(sm, model, meta, depth)
        del keep
    finally:
        reset(gm, sm)


def _top_runs():
    """two TCP streams of 3 302 and 3 301 members, captured in a random order (the module docstring says what they hold)"""
    rng = np.random.default_rng(42)
    m, x = 3300, 16
    top = BOUND - x - 200                                           # where the covering member starts; it ends at 2^31 - 1 - x
    a = [(0, b"head"), (top, bytes(rng.integers(1, 256, 200, dtype=np.uint8)))]
    for _ in range(m - 1):
        o = int(rng.integers(1, 200))
        a.append((top + o, bytes(rng.integers(1, 256, int(rng.integers(0, 200 - o + 1)), dtype=np.uint8))))
    a.append((top + 195, bytes(rng.integers(1, 256, 10, dtype=np.uint8))))      # 5 bytes covered, 5 kept
    b = [(0, b"head")] + [(BOUND - 2 * m + 2 * i + 1, bytes(rng.integers(1, 256, 1, dtype=np.uint8))) for i in range(m)]
    rows, pay, seq = [], [], []
    for row, segs, isn in ((X, a, 0xFFFFFF00), (Z, b, 0x7FFFFFF0)):
        for j in rng.permutation(len(segs)):
            rows.append(row)
            pay.append(segs[j][1])
            seq.append((isn + segs[j][0]) & 0xFFFFFFFF)
    order = rng.permutation(len(rows))                              # the two streams' members interleaved
    return [rows[i] for i in order], [pay[i] for i in order], np.array(seq, dtype=np.uint32)[order], m


def test_one_stream_across_scan_tiles(gm, sm):
    rows, pay, seq, m = _top_runs()
    meta = _meta(rows)
    model = QM.build(pay, meta, seq, FULL)
    recs, segs, orders = model[1], model[3], model[4]
    lens = np.array([len(t) for t in pay])
    assert sorted(recs["n_packets"].tolist()) == [m + 1, m + 2] and sorted(recs["bytes"].tolist()) == [4 + 200 + 5, 4 + m]
    assert ((segs["take"] == 0) & (lens > 0)).sum() > m - 200 and sorted(orders["n_gaps"].tolist()) == [1, m]
    assert sorted(orders["gap_bytes"].tolist()) == [BOUND - 4 - m, BOUND - 16 - 200 - 4] and max(len(t) for t in pay) == 200
    reset(gm, sm)
    gm.set_patterns([b"x"])
    load(gm, pay)
    gm.set_meta(meta)
    gm.build_flows()
    for depth in (FULL, 207, 1000):
        assert sm.load_streams(gm, depth, seq=seq) == 2
        check(sm, model, meta, depth)


def test_offsets_map_back_across_the_holes(gm, sm):
    """stream_locate_ordered at the first and last kept byte of every member that kept one -- the members on both sides of every stream's
    largest hole among them -- against the model's origin"""
    pay, meta, seq, model = wide()
    streams, recs, pos, segs, orders, origin = model
    reset(gm, sm)
    gm.set_patterns([b"x"])
    load(gm, pay)
    gm.set_meta(meta)
    gm.build_flows()
    sm.load_streams(gm, FULL, seq=seq)
    smap, gsegs = sm.stream_map(), sm.stream_segs()
    kept = np.flatnonzero(segs["take"] > 0)
    around = []                                                     # the members in front of and behind the largest hole of every TCP stream
    for s in np.flatnonzero(orders["tcp"] == 1):
        ks = kept[pos["stream"][kept] == s]
        ks = ks[np.argsort(pos["pos"][ks])]
        end = segs["seq_off"][ks].astype(np.int64) + segs["skip"][ks] + segs["take"][ks]
        hole = segs["seq_off"][ks][1:].astype(np.int64) + segs["skip"][ks][1:] - end[:-1]
        if hole.size and hole.max() > 0:
            j = int(np.argmax(hole))
            around += [(int(ks[j]), int(hole[j])), (int(ks[j + 1]), int(hole[j]))]
    assert len(around) >= 20 and max(h for _, h in around) > 1 << 30
    ks = np.concatenate([kept, kept])
    at = np.concatenate([pos["pos"][kept], pos["pos"][kept] + segs["take"][kept] - np.uint64(1)])
    assert {k for k, _ in around} <= set(ks.tolist())
    k, j = stream_locate_ordered(smap, gsegs, pos["stream"][ks], at)
    want = [origin[int(s)][int(x)] for s, x in zip(pos["stream"][ks], at)]
    assert list(zip(k.tolist(), j.tolist())) == want
    assert k.tolist() == ks.tolist() and j[:len(kept)].tolist() == segs["skip"][kept].tolist()
    assert j[len(kept):].tolist() == [len(pay[int(i)]) - 1 for i in kept]


def test_semantics_across_a_wide_hole(gm, sm):
    """What closing holes and dropping covered bytes mean for a scan, at the bound: a content whose halves lie on either side of a hole of
    almost 2^31 is found in the stream; a content that stands only in a covered retransmission's own bytes is not."""
    far = BOUND - 12
    pay = [b"CONTENT tail", b"0123456789", b"....SPLIT", b"xxHIDDENx", b"answer"]
    rows = [X, X, X, X, Z]
    seq = (0xFFFFFFF0 + np.array([far, 0, 10, 10, 0], dtype=np.uint64)).astype(np.uint32)         # member 3, captured behind 2, is covered by it
    pats = [b"SPLITCONTENT", b"HIDDEN", b"answer", b"0123456789"]
    meta = _meta(rows)
    model = QM.build(pay, meta, seq, FULL)
    assert model[0] == [b"0123456789....SPLITCONTENT tail", b"answer"] and model[4]["gap_bytes"].tolist() == [far - 19, 0]
    assert model[3]["seq_off"].tolist() == [far, 0, 10, 10, 0] and far + len(pay[0]) == BOUND
    want = MM.counts(MM.starts(model[0], pats))
    assert want == [1, 0, 1, 1]
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns(pats)
    load(gm, pay)
    gm.set_meta(meta)
    assert gm.build_flows() == 2
    assert gm.scan()[0].tolist() == [0, 1, 1, 1]                    # the payloads themselves: the split content is in none, HIDDEN in one
    sm.load_streams(gm, FULL, seq=seq)
    check(sm, model, meta, FULL)
    assert sm.scan()[0].tolist() == want
    sm.load_streams(gm, FULL)                                       # capture order: neither closes the hole nor drops the copy
    assert sm.scan()[0].tolist() == MM.counts(MM.starts(TM.payloads(pay, meta, FULL), pats)) == [0, 1, 1, 1]
