"""kmpgpu_load_selected, kmpgpu_load_decoded and kmpgpu_load_streams WRITING arenas across and behind offset 2^32, on a real MI355X.

Half of a 12 GB capture selected is 6 GB, a decoded capture is about its own size, the streams of one are up to its size: in real use all
three write above 2^32, and the suite's destinations were a few MiB (the sources alone reached 2^32: test_gpu_select.py::
test_source_past_4_gib, test_gpu_decode.py::test_high_offsets, test_gpu_streams_scale.py::test_source_on_both_sides_of_2_32, the seam rows
of test_gpu_high_offsets.py).  Here every destination ends above 2^32 + 2^27, asserted in each test.

The source is periodic: payload k is entry k % 257 of a period of 257 payloads that a test chooses, laid out ON THE DEVICE by torch
(gpu_support.periodic_source: nothing of 4 GiB is built on the host or uploaded) and borrowed in place by one context (the `source`
fixture).  What dst has to hold is periodic too and follows from the period by index arithmetic (gpu_support.periodic_dst): index,
offsets and lengths are compared in full, the downloaded arena by one reshape to [periods, period bytes] against the period's image, the
incomplete period and the 64 bytes of 0x00 behind the end apart.  Every payload of 8 bytes and more begins with prep_model.tag(k % 257)
-- no '%', no '+', so it survives the decoding; in every member of a stream -- and a count of the 257 tags over dst under the auto, packed
and fused kernels pins every payload once more, through the start bitmap and pad_clean = true of an arena the library built itself.  For
the streams the bytes of 77 whole streams are compared (the one that holds byte 2^32 with two neighbours on either side, the first and
last four, 64 random ones); everything else of the 4.7 GB is held by records, map, off and len in full and by the tag counts in closed form
(a tag stands in a member's first 8 bytes and in no other place, so it counts where pos + 8 <= len of its stream).
tests/test_high_destinations_model.py holds all of these expectations to prep_model.gather_slots, decode_model.load_decoded and
stream_model on three periods and a rest, and the device layout (torch on the CPU) to decode_model.packed_image.  No nocase pattern
anywhere: the fold buffer would add 4 GiB.

Address arithmetic read before the first run, for destination offsets of 2^32 and more (csrc/):
    kmp_select.hip   kmp_select_index_kernel: pkt_off[j] = blk_bytes[blk] + loc_off[k], both uint64.  kmp_select_copy_kernel: base, end, d0 and
                     d uint64, the lane's share `(uint64_t)lane * 16u`, s_off[] uint64 in LDS with ~0 behind the run, rel = d - s_off[p] a
                     64-bit difference compared with the 32-bit length, dst + d.  Clean.
    kmp_decode.hip   kmp_decode_index_kernel as the select one.  kmp_decode_write_kernel: the empty payload's slot at dst + off with
                     off + 16 <= total in 64 bits; straight copy d = doff + before with doff uint64 from LDS; staged path
                     out = doff + before, a0 = bcast64(out, 0) & ~15ull, pos = (uint32_t)(out - a0) (a difference below the stage's size),
                     d = a0 + 16ull * t, every guard d + 16 <= total in 64 bits.  Clean.
    kmp_streams.hip  kmp_stream_index_kernel: pkt_off[s] and piece_dst[i] = blk_bytes[..] + loc_off[s] (+ at) uint64, pos a difference of
                     64-bit sums written as two 32-bit halves; kmp_stream_records_kernel: bytes uint64 into the 64-bit record word;
                     kmp_stream_gather_kernel: u, span and u_end uint64, d = u * 16u in 64 bits, advance_piece over uint64 keys with a
                     32-bit piece number (n < 2^32 payloads), d - pd < 2^30 or -15 .. -1, dst + u * 16u.  Clean.
    kmp_prep.hip     kmp_scan_local_kernel / kmp_scan_totals_kernel behind all three: 64-bit byte sums (held past 2^32 by
                     test_gpu_prep_scale.py::test_arena_past_4_gib); kmp_validate_index_kernel as in test_gpu_high_offsets.py.  Clean.
    matcher.py       stream_locate: uint64 keys, base = cumsum(last_pos + 1) in uint64.  Clean.
Nothing wrong was found by reading, and no byte came out wrong.

What the tests found.
  1. test_stream_longer_than_2_32 showed a gap between two contracts.  include/kmpgpu.h allows depths of 1 .. KMPGPU_STREAM_DEPTH_MAX =
     2^30, and kmp_validate_index_kernel took lengths BELOW 2^30 only: a stream that reached 2^30 bytes under depth 2^30 was built and then
     refused -- "kmpgpu_load_streams failed (-2): kmpgpu_load_streams: a payload length is not below 2^30", dst left empty.  Every stream
     the suite had cut at 2^30 was shorter.  Fixed in csrc/: the layout check (kmp_validate_index_kernel, and the host loop of
     kmpgpu_load_arena) now takes lengths up to 2^30 and refuses what is above.  Read for the one new value: every position inside a
     payload stays below 2^31 (what kmpgpu.h gives as the reason for the depth's bound); kmp_scan_general.hip keeps a chunk's offset in
     30 bits beside two flags, and a chunk starts below the length, so at most at 2^30 - KMP_CHUNK; a packed range is a plan step below
     2^30 plus a slot of at most 2^30, below 2^31; the flat kernel's ppw * stride is 2^30.  The test counts three tags in the 2^30-byte
     payload under the auto, packed, fused and general kernels; test_gpu_prep_scale.py::test_layout_check_on_the_device now refuses
     2^30 + 1.
  2. The serial walk behind a cut that is no multiple of 16 (kmp_stream_gather_kernel, `do .. while (pd < d + 16)`): one stream of
     800 000 members of 1 458 bytes, 100 000 of them behind the cut -- kernel_ms 22.217 at depth 1 020 599 993, 0.944 at 1 020 599 984: 213 ns
     per member behind the cut, one lane.  A linear estimate for the 2.4 M members behind a cut of the long stream is 0.51 s; that shape was
     not run.  profiles/streams.txt, DESIGN.md section 8, item 7.  No test asserts on a time; the kernel is as it was.

Memory.  Device: the source 4.7 .. 7.0 GB (decoded, changed payloads only, needs 2.31 M source payloads), dst 4.4 .. 4.7 GB plus an eighth of
headroom, scratch below 0.5 GB: a peak of about 12.5 GB in test_decoded_past_2_32 and 10 .. 11 GB in the others; the uniform source of
test_selected_past_2_32 is built after the mixed one was given back.  Host: one download of up to 4.74 GB at a time; each test is skipped
where MemAvailable is under twice its download -- the module's only skip.

Run on a real MI355X:  python -m pytest tests/test_gpu_high_destinations.py -m gpu
Measured there (each test in a process of its own, call time): test_selected_past_2_32 4.5 s (three destinations of 4.43 GB),
test_decoded_past_2_32 2.9 s (two), test_streams_past_2_32 4.3 s (4.74 and 4.49 GB), test_stream_longer_than_2_32 6.1 s (three
destinations of 1 GiB and four scans of a payload that is one wavefront's under the streaming kernels).

Checked to bite, as test_gpu_high_offsets.py was: memory-safe changes to scratch builds (never committed), each of which cuts ONE
destination offset to its low 32 bits -- the wrong address then lies in the low part of the same dst allocation -- and each run once over
this module.  None cuts piece_dst, s_off or a loop bound.
  1  kmp_select_index_kernel, pkt_off[j] = (uint32_t)(..)       test_selected_past_2_32: 46 108 789 bytes of periods 0 .. 127 differ, the first
                                                                at 17 792 (the library repacks the overlapping slots, so off passes)
  2  kmp_select_copy_kernel, dst + (uint32_t)d                  test_selected_past_2_32: 46 303 488 bytes of periods 0 .. 127 differ, from byte 0
  3  kmp_decode_write_kernel, staged path, a0 cut               test_decoded_past_2_32: 68 479 278 bytes of periods 0 .. 127 differ, the first at 320
  4  kmp_decode_write_kernel, straight copy, d cut              test_decoded_past_2_32: 24 578 208 bytes of periods 0 .. 127 differ, the first at 5 056
  5  kmp_stream_gather_kernel, dst + (uint32_t)(u * 16u)        test_streams_past_2_32: stream 0 differs from its byte 0
  6  kmp_stream_index_kernel, high word of pos written as 0     test_stream_longer_than_2_32: the map differs from member 2 945 794 on
  7  kmp_stream_records_kernel, bytes cut                       test_stream_longer_than_2_32: record 0 differs (byte 28, the high word of bytes)
Every other test of the module passed on each build (builds 1 to 5 were run before the layout check took 2^30, when
test_stream_longer_than_2_32 still stopped at the refusal; 6 and 7 were run again over that test behind the fix, with the figures above).
A build with all seven changes at once was run once over test_gpu_select.py, test_gpu_decode.py, test_gpu_decode_scale.py, test_gpu_streams.py and test_gpu_streams_scale.py: 130 passed,
2 skipped -- the gap this module closes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import (B32, EMPTY_ARENA, FLOW_A, FLOW_B, PERIOD, PeriodicSource, check_periodic_bytes, meta_of_flows,  # noqa: E402  (torch first)
                         period_image, periodic_dst, reset, tag_counts, tagged)

import decode_model as DM  # noqa: E402
import prep_model as PM  # noqa: E402
import stream_model as TM  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_FLAT, KERNEL_GENERAL, KERNEL_PACKED, OPT_NONTEMPORAL, GpuMatcher, stream_locate)
from test_gpu_decode_scale import expectation, period as decode_period  # noqa: E402
from test_gpu_prep_scale import KERNEL_FUSED, _mem_available, _scan  # noqa: E402
from test_gpu_streams_scale import expected_arena  # noqa: E402

HIGH = B32 + (1 << 27)                     # every destination of this module ends above it
TAGS = [PM.tag(e) for e in range(PERIOD)]
FAMILIES = (KERNEL_AUTO, KERNEL_PACKED, KERNEL_FUSED)
REST = 100                                 # payloads of the last, incomplete period
SELECT_LENS = {9000: 30, 1500: 82, 48: 30, 17: 30, 16: 30, 15: 25, 1: 15, 0: 15}      # length: entries of the period; the mean slot is 1 546 bytes
N_FLOWS = 3000
N_STREAMS = 6_400_000                      # payloads of 1 458 and 17 bytes in turn: 4.74 GB of streams, 4.49 GB with every forward stream cut
MEMBER = 1458
N_LONG, N_SHORT, BEHIND = 3_100_003, 800_000, 100_000
assert sum(SELECT_LENS.values()) == PERIOD


# ------------------------------------------------------------------------------------------------
# the periods and the expectations: numpy, no device (tests/test_high_destinations_model.py holds them to the plain models)
# ------------------------------------------------------------------------------------------------
def filler(rng, L):
    return rng.integers(0x61, 0x7B, L, dtype=np.uint8).tobytes()


def periods_above(dst_period_bytes, more=0):
    """whole periods of a destination that bring its end above HIGH"""
    return -(-(HIGH + (1 << 20)) // dst_period_bytes) + more


def select_period():
    """(257 payloads of the lengths of SELECT_LENS in shuffled order, every one of 8 bytes and more under its tag; the period of the bitmap:
    about 0.9 dense, entries 0 and 256 unselected)"""
    rng = np.random.default_rng(2032)
    lens = np.repeat(list(SELECT_LENS), list(SELECT_LENS.values()))
    rng.shuffle(lens)
    pay = [tagged(filler(rng, int(L)), e) for e, L in enumerate(lens)]
    psel = rng.random(PERIOD) < 0.9
    psel[0] = psel[PERIOD - 1] = False
    return pay, psel


def uniform_period():
    rng = np.random.default_rng(2033)
    return [tagged(filler(rng, 1500), e) for e in range(PERIOD)], np.ones(PERIOD, dtype=bool)


def selection(pay, psel, n):
    """what kmpgpu_load_selected leaves of the periodic source of n payloads under the bitmap psel[k % 257]"""
    index = np.flatnonzero(psel)
    want = periodic_dst(period_image([pay[int(i)] for i in index]), index, n)
    reps, rest = divmod(n, PERIOD)
    want["sel"] = psel[np.arange(n) % PERIOD]
    want["tags"] = tag_counts(pay, np.where(psel, reps + (np.arange(PERIOD) < rest), 0))
    return want


def decode_base():
    """the period of tests/test_gpu_decode_scale.py ("large"), every payload under its tag"""
    return [tagged(t, e) for e, t in enumerate(decode_period("large"))]


def decoded(base, n, plus, only_changed):
    """what kmpgpu_load_decoded leaves and hands out over the periodic source of n payloads: one period by test_gpu_decode_scale.expectation
    (tests/decode_model.py), the others by index arithmetic"""
    one = expectation(base, PERIOD, plus, only_changed)
    want = periodic_dst((one["arena"], one["off"], one["len"]), one["index"], n)
    reps, rest = divmod(n, PERIOD)
    src_len = np.array([len(t) for t in base], dtype=np.int64)
    want["changed"] = np.concatenate([np.tile(one["changed"], reps), one["changed"][:rest]])
    want["stats"] = {"n_payloads": len(want["len"]), "n_changed": int(want["changed"].sum()),
                     "bytes_in": int(src_len[want["index"] % PERIOD].sum()), "bytes_out": int(want["len"].sum(dtype=np.uint64))}
    out = [DM.decode(base[int(e)], plus) for e in one["index"]]
    want["tags"] = tag_counts(out, reps + (one["index"] < rest))
    return want


def write_paths(base):
    """(entries without a '%' and a '+': every step of theirs is the straight copy; entries with an escape in a 16-byte unit whose first
    byte goes to an output position that is no multiple of 16: the staged path)"""
    straight, staged = [], []
    for e, t in enumerate(base):
        p = np.frombuffer(t, dtype=np.uint8)
        esc = DM.escapes(p)
        if b"%" not in t and b"+" not in t:
            straight.append(e)
        consumed = np.zeros(p.size, dtype=bool)
        consumed[1:] |= esc[:-1]
        consumed[2:] |= esc[:-2]
        out = np.cumsum(~consumed) - ~consumed                         # where every source byte goes
        if any(out[16 * (int(i) // 16)] % 16 for i in np.flatnonzero(esc)):
            staged.append(e)
    return straight, staged


def stream_period(alternate=True):
    """257 payloads of 1 458 bytes, every other one of 17 where `alternate`, each under its tag, no 0x00 and no '<' behind the tag: a tag
    is found once per member that lies in front of the cut with its first 8 bytes, and nowhere across two members"""
    rng = np.random.default_rng(2034)
    pay = [tagged(filler(rng, 17 if alternate and e % 2 else MEMBER), e) for e in range(PERIOD)]
    assert all(t.startswith(PM.tag(e)) and b"<" not in t[1:] and b"\0" not in t for e, t in enumerate(pay))
    return pay


def flows_of(n, n_flows=N_FLOWS):
    """the metadata of n payloads: a multiplicative hash of k into n_flows flows, every third payload of a flow the answer; every flow
    opens with a payload that is none, so its direction 0 is the forward one, with two thirds of its payloads"""
    k = np.arange(n, dtype=np.int64)
    flow = (k * 2654435761 >> 7) % n_flows
    meta = meta_of_flows(flow, seed=4)
    first = np.unique(flow, return_index=True)[1]
    meta["src_ip"][first], meta["dst_ip"][first] = FLOW_A + flow[first], FLOW_B
    meta["src_port"][first], meta["dst_port"][first] = 1000 + flow[first] % 7, 53
    return meta


def cut_to(recs, depth):
    """the records of the same streams under another depth: only len depends on it"""
    out = recs.copy()
    out["len"] = np.minimum(recs["bytes"], depth)
    return out


def period_lens(pay, n):
    return np.array([len(t) for t in pay], dtype=np.uint32)[np.arange(n) % PERIOD]


def stream_index(recs):
    """(off, slot size) of the packed streams, int64"""
    size = PM.slot_bytes(recs["len"]).astype(np.int64)
    return np.cumsum(size) - size, size


def stream_tag_counts(recs, pos, tag_len=8):
    """counts[t] over the stream arena, in closed form: member k holds tag(k % 257) in its first 8 bytes, and those lie in front of the
    cut where pos + 8 <= len of its stream"""
    st = pos["stream"].astype(np.int64)
    whole = pos["pos"].astype(np.int64) + tag_len <= recs["len"].astype(np.int64)[st]
    return np.bincount((np.arange(len(pos)) % PERIOD)[whole], minlength=PERIOD)


def streams_bytes(image, lens, recs, pos, chosen):
    """(bytes, off[len(chosen)]) of the packed streams `chosen` (ascending) alone: test_gpu_streams_scale.expected_arena over their members,
    whose bytes come from the period's image"""
    img, poff, _ = image
    chosen = np.asarray(chosen, dtype=np.int64)
    ks = np.flatnonzero(np.isin(pos["stream"], chosen))
    sub = pos[ks].copy()
    sub["stream"] = np.searchsorted(chosen, sub["stream"])
    want, woff, _ = expected_arena(img, poff[ks % PERIOD], lens[ks], recs[chosen], sub)
    return want, woff.astype(np.int64)


def chosen_streams(soff, n_streams, seed=5):
    """the stream that holds byte 2^32 with two neighbours on either side, the first four, the last four and 64 random ones"""
    s32 = int(np.searchsorted(soff, B32, side="right")) - 1
    rng = np.random.default_rng(seed)
    return s32, np.unique(np.concatenate([np.arange(s32 - 2, s32 + 3), np.arange(4), np.arange(n_streams - 4, n_streams),
                                          rng.integers(0, n_streams, 64)]))


# ------------------------------------------------------------------------------------------------
# the device side
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def source():
    """the big source: one context, whose borrowed arena every test lays out on the device for its own period (PeriodicSource.build)"""
    s = PeriodicSource()
    yield s
    s.close()


class Destination:
    """one dst context per test, its arena given back at the end"""

    def __init__(self, patterns=TAGS):
        self.patterns = patterns

    def __enter__(self):
        self.m = GpuMatcher(0)
        self.m.set_patterns(self.patterns)
        return self.m

    def __exit__(self, *exc):
        try:
            self.m.load_arena(*EMPTY_ARENA)
            assert self.m.arena_info() == (0, 0)
        finally:
            self.m.close()


def host_can_hold(download):
    if _mem_available() < 2 * download:
        pytest.skip(f"MemAvailable is under twice the download of {download} bytes")


def check_index_and_bytes(dst, want):
    """arena_info, off and len in full, every byte of the arena, then the tag counts under the three kernel families"""
    assert want["end"] > HIGH
    assert dst.arena_info() == (len(want["len"]), int(want["len"].sum(dtype=np.uint64)))
    a, off, ln = dst.arena_download()
    assert np.array_equal(off, want["off"]), np.flatnonzero(off != want["off"])[:4]
    assert np.array_equal(ln, want["len"]), np.flatnonzero(ln != want["len"])[:4]
    check_periodic_bytes(a, want)


def check_tags(dst, tags, kernels=FAMILIES):
    for kernel in kernels:
        got = _scan(dst, kernel)
        assert got.tolist() == np.asarray(tags).tolist(), (kernel, [(t, int(got[t]), int(tags[t])) for t in np.flatnonzero(got != tags)[:4]])


def test_selected_past_2_32(source):
    """kmpgpu_load_selected with a destination of 4.45 GB: the mixed lengths under both instantiations of the copy kernel (runs of 8 and
    fewer payloads by the mean slot; 16-byte slots and 9 000-byte payloads behind 2^32), then the uniform source with every bit set"""
    pay, psel = select_period()
    lens = np.array([len(t) for t in pay])
    assert all((psel & (lens == L)).any() for L in SELECT_LENS) and 15 <= (~psel).sum() <= 40 and (~psel & (lens >= 1500)).any()
    n = periods_above(len(period_image([t for t, s in zip(pay, psel) if s])[0])) * PERIOD + REST
    want = selection(pay, psel, n)
    host_can_hold(want["end"] + 64)
    assert 2_900_000 < n < 3_400_000 and not np.array_equal(want["index"], np.arange(len(want["index"])))
    src = source.build(pay, n)
    with Destination() as dst:
        for nontemporal in (1, 0):
            dst.set_option(OPT_NONTEMPORAL, nontemporal)
            idx = dst.load_selected(src, want["sel"])
            assert np.array_equal(idx.astype(np.int64), want["index"])
            check_index_and_bytes(dst, want)
            check_tags(dst, want["tags"])
        pay, psel = uniform_period()
        n = periods_above(PERIOD * 1504) * PERIOD + REST
        want = selection(pay, psel, n)
        assert want["index"].size == n and want["tags"].sum() == n
        src = source.build(pay, n)
        idx = dst.load_selected(src, want["sel"])
        assert np.array_equal(idx.astype(np.int64), want["index"])
        check_index_and_bytes(dst, want)
        check_tags(dst, want["tags"], FAMILIES + (KERNEL_FLAT,))
    source.release()


def test_decoded_past_2_32(source):
    """kmpgpu_load_decoded with destinations of 4.45 GB: everything decoded, and the changed payloads alone with '+' (a longer source); the
    straight copy and the staged path both write behind 2^32"""
    base = decode_base()
    straight, staged = write_paths(base)
    assert len(straight) > PERIOD // 4 and len(staged) > PERIOD // 4
    modes = []
    for plus, only_changed, nontemporal in ((False, False, 1), (True, True, 0)):
        one = expectation(base, PERIOD, plus, only_changed)
        n = periods_above(len(one["arena"]), more=1) * PERIOD + REST
        want = decoded(base, n, plus, only_changed)
        # the first full period behind 2^32 is not the last one, and it holds payloads of both write paths
        first = -(-B32 // len(want["per"]))
        assert first < want["reps"] and set(staged) & set(one["index"].tolist())
        assert only_changed or set(straight) & set(one["index"].tolist())
        assert want["stats"]["bytes_in"] > B32 and want["stats"]["bytes_out"] > B32 and 0 < want["stats"]["n_changed"] < n
        modes.append((plus, only_changed, nontemporal, n, want))
    host_can_hold(max(m[4]["end"] for m in modes) + 64)
    assert 1_400_000 < modes[0][3] < 1_700_000 < modes[1][3]
    source.build(base, max(m[3] for m in modes))
    with Destination() as dst:
        for plus, only_changed, nontemporal, n, want in modes:
            src = source.use(n)
            dst.set_option(OPT_NONTEMPORAL, nontemporal)
            res = dst.load_decoded(src, plus=plus, only_changed=only_changed)
            assert np.array_equal(res["changed"], want["changed"]) and np.array_equal(res["index"], want["index"])
            assert res["stats"] == want["stats"]
            check_index_and_bytes(dst, want)
            check_tags(dst, want["tags"])
    source.release()


def check_stream_records(dst, recs, pos, meta):
    got, gmap = dst.streams(), dst.stream_map()
    assert got.tobytes() == recs.tobytes(), np.flatnonzero(got != recs)[:4]
    assert gmap.tobytes() == pos.tobytes(), np.flatnonzero(gmap != pos)[:4]
    assert dst.meta().tobytes() == meta[recs["first_packet"].astype(np.int64)].tobytes()


def test_streams_past_2_32(source):
    """kmpgpu_load_streams with destinations of 4.5 GB and more: about 6 000 streams of 0.5 to 1 MB, uncut and with every forward stream
    cut"""
    pay = stream_period()
    image = period_image(pay)
    n = N_STREAMS
    lens, meta = period_lens(pay, n), flows_of(n)
    uncut, pos = TM.records_np(meta, lens, 1 << 30)
    forward = uncut["bytes"][uncut["dir"] == 0]
    cut = (int(forward.min()) - 1) // 16 * 16
    assert cut % 16 == 0 and (forward > cut).all() and (uncut["bytes"][uncut["dir"] == 1] < cut).all()
    assert len(uncut) == 2 * N_FLOWS and 400_000 < uncut["bytes"].min() and uncut["bytes"].max() < 1_300_000
    host_can_hold(int(stream_index(uncut)[1].sum()) + 64)
    src = source.build(pay, n)
    src.set_meta(meta)
    assert src.build_flows() == N_FLOWS
    with Destination() as dst:
        for depth in (1 << 30, cut):
            recs = cut_to(uncut, depth)                                # (the map does not depend on the depth)
            soff, size = stream_index(recs)
            end = int(size.sum())
            assert end > HIGH and (depth == cut) == bool((recs["bytes"] > recs["len"]).any())
            assert dst.load_streams(src, depth) == len(recs)
            check_stream_records(dst, recs, pos, meta)
            assert dst.arena_info() == (len(recs), int(recs["len"].sum(dtype=np.uint64)))
            a, off, ln = dst.arena_download()
            assert np.array_equal(off, soff.astype(np.uint64)) and np.array_equal(ln, recs["len"])
            assert len(a) == end + 64 and not a[end:].any()
            s32, chosen = chosen_streams(soff, len(recs))
            assert soff[s32] <= B32 < soff[s32] + size[s32] and chosen[0] == 0 and chosen[-1] == len(recs) - 1 and len(chosen) >= 64
            assert (chosen < s32 - 2).sum() >= 8 and (chosen > s32 + 2).sum() >= 8            # whole streams on both sides of 2^32
            want, woff = streams_bytes(image, lens, recs, pos, chosen)
            for j, s in enumerate(chosen.tolist()):
                o, z, w = int(soff[s]), int(size[s]), int(woff[j])
                assert np.array_equal(a[o:o + z], want[w:w + z]), (s, o, int(np.flatnonzero(a[o:o + z] != want[w:w + z])[0]))
            del a, want
            # every other byte: a count of every member's tag over the whole arena
            tags = stream_tag_counts(recs, pos)
            assert (tags.sum() == n) == (depth != cut) and tags.min() > 0
            check_tags(dst, tags)
    source.release()


class LongStream:
    """one flow with every payload in one direction: a single stream of n members of 1 458 bytes over the periodic source"""

    def __init__(self, source):
        self.source = source
        self.pay = stream_period(alternate=False)
        self.whole = np.frombuffer(b"".join(self.pay), dtype=np.uint8)  # one period of the stream's bytes
        self.one = meta_of_flows(np.zeros(1, dtype=np.int64), seed=4)
        host_can_hold((1 << 30) + 64)
        source.build(self.pay, N_LONG)

    def run(self, dst, n, depth):
        """load_streams of the first n payloads; records, map, index and every byte of the stream.  Returns (the map, kernel_ms)."""
        meta, lens, whole = np.repeat(self.one, n), period_lens(self.pay, n), self.whole
        m = self.source.use(n)
        m.set_meta(meta)
        assert m.build_flows() == 1
        recs, pos = TM.records_np(meta, lens, depth)
        assert dst.load_streams(m, depth) == 1
        ms = dst.last_timing().kernel_ms
        check_stream_records(dst, recs, pos, meta)
        assert recs["bytes"].tolist() == [n * MEMBER] and recs["len"].tolist() == [depth] and recs["n_packets"].tolist() == [n]
        assert dst.arena_info() == (1, depth)
        a, off, ln = dst.arena_download()
        assert off.tolist() == [0] and ln.tolist() == [depth]
        assert len(a) == (depth + 15) // 16 * 16 + 64 and not a[depth:].any()
        reps = depth // len(whole)
        assert (a[:reps * len(whole)].reshape(reps, len(whole)) == whole).all()
        assert np.array_equal(a[reps * len(whole):depth], whole[:depth - reps * len(whole)])
        return dst.stream_map(), ms

    def check_high_words(self, gmap, depth):
        """bytes and pos above 2^32, and stream_locate in front of and at the cut and on both sides of 2^32"""
        assert N_LONG * MEMBER > HIGH
        k32 = -(-B32 // MEMBER)                                        # the first member whose pos has a high word
        assert k32 == 2_945_794 and int(gmap["pos"][k32 - 1]) < B32 <= int(gmap["pos"][k32]) and int(gmap["pos"][-1]) == (N_LONG - 1) * MEMBER
        at = np.array([0, depth - 1, depth, B32 - 1, B32, B32 + 1, k32 * MEMBER - 1, k32 * MEMBER, N_LONG * MEMBER - 1], dtype=np.uint64)
        k, o = stream_locate(gmap, np.zeros(len(at), dtype=np.uint64), at)
        assert k.tolist() == (at // np.uint64(MEMBER)).tolist() and o.tolist() == (at % np.uint64(MEMBER)).tolist()


LONG_TAGS = (0, 128, 256)                  # the tags counted over the one long stream: a payload of 1 GiB is one wavefront's under some kernels


def test_stream_longer_than_2_32(source):
    """One stream of 3.1 M members of 1 458 bytes, 4.52e9 bytes, under depth 2^30 = KMPGPU_STREAM_DEPTH_MAX: bytes and the pos of every
    member from 2 945 794 on have a set high word, and the stream is a payload of exactly 2^30 bytes -- the longest an arena takes
    (kmp_validate_index_kernel), which the scan kernels of every family then count three tags in.  Then a cut that is no multiple of 16
    with 100 000 members behind it, whose pieces all start inside the stream's last unit: one lane of the gather visits them one after the
    other.  That call's kernel time and the one of the cut rounded down are printed, not asserted on."""
    long = LongStream(source)
    with Destination([TAGS[t] for t in LONG_TAGS]) as dst:
        depth = 1 << 30
        gmap, _ = long.run(dst, N_LONG, depth)
        long.check_high_words(gmap, depth)
        behind = int((gmap["pos"].astype(np.int64) + 8 <= depth).sum())                  # members whose tag lies in front of the cut
        want = [(behind - t + PERIOD - 1) // PERIOD for t in LONG_TAGS]
        assert behind == (depth - 8) // MEMBER + 1 and sum(want) > 8000
        for kernel in FAMILIES + (KERNEL_GENERAL,):
            assert _scan(dst, kernel).tolist() == want, kernel
        reset(dst)
        odd = (N_SHORT - BEHIND) * MEMBER - 7
        assert odd % 16 and odd < (1 << 30)
        for depth in (odd, odd // 16 * 16):
            _, ms = long.run(dst, N_SHORT, depth)
            print(f"kmpgpu_load_streams, one stream of {N_SHORT} members of {MEMBER} bytes, depth {depth} (% 16 = {depth % 16}), "
                  f"{BEHIND} members behind the cut: kernel_ms {ms:.3f}")
    source.release()


