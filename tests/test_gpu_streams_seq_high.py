"""kmpgpu_load_streams_ordered WRITING past 2^32 and summing past it, on a real MI355X: the ordered call's share of
tests/test_gpu_high_destinations.py, which was written one commit before the call existed.  The suite's destinations of the ordered call
were a few MiB, no stream of it had reached depth = 2^30, and no take-sum, pos or bytes of it had a set high word.  Here every destination
ends above HIGH = 2^32 + 2^27, asserted in each test.

Method, memory discipline and helpers are the sibling's: the source is periodic (payload k is entry k % 257 of a period), laid out ON THE
DEVICE by gpu_support.PeriodicSource -- nothing of 4 GiB is built on the host -- and borrowed in place; one destination context per test,
given back with EMPTY_ARENA; a test is skipped only where MemAvailable is under twice its download; no nocase pattern.

  test_ordered_streams_past_2_32     Period r (257 payloads of 1 458 bytes, every other one 17, each under its prep_model.tag) lies in 6
      flows of its own, both directions, one flow UDP; inside a period every TCP stream's members are permuted, duplicated, overlapping and
      gapped (segment_offsets, the shape of test_gpu_streams_seq._segments over given lengths).  So everything dst has to hold is
      stream_seq_model.build of ONE period, and of the period's first 100 payloads for the rest, tiled with the indices moved on (tiled):
      records, map, segs, orders, off, len and metadata are compared in full, the arena byte for byte by one reshape to
      [periods, period bytes], then the incomplete period and the 64 bytes of 0x00 behind the end.  2^32 is no multiple of the period's
      bytes, so a write displaced by 2^32 cannot land on equal bytes.  The 257 tags are counted under the auto, packed and fused kernels
      against gpu_support.tag_counts over the model's streams: a tag inside a covered front does not count.  The issue that asked for this
      test spoke of about 3.2 M payloads; with every other payload 17 bytes long and part of the rest dropped as retransmitted, a period
      keeps 182 KB under the cut depth, and a destination above HIGH takes 6 254 452 payloads (24 336 periods, 146 022 flows,
      292 044 streams) -- the payload count follows from the bound on the destination, which is what the test is about.
  test_long_udp_stream_through_the_ordered_call     LongStream of the sibling, one stream of 3 100 003 members, proto 17, through the ordered
      call with arbitrary nonzero seq: what kmpgpu_load_streams gives (LongStream's checks, check_high_words), orders all zero, segs
      {0, 1458, 0}; bytes = 4.52e9, pos with a set high word from member 2 945 794 on, len exactly 2^30.  Then 800 000 members with
      100 000 behind an odd cut and behind the cut rounded down to 16: the kernel times of both calls are printed beside those of
      kmpgpu_load_streams, not asserted on.
  test_long_tcp_stream_to_the_depth     One TCP stream on a schedule over each ten consecutive payloads (schedule): payload 4 an exact
      retransmission of 3, payload 7 starting 100 bytes before the end of 6, 8 and 9 swapped in capture order, a 3-byte hole in front of
      every group.  A group keeps 9 * 1458 - 100 = 13 022 bytes, so the 800 000 members the issue names keep 1.04e9 bytes, which is BELOW
      2^30; the stream has 830 000 members (1.08e9 of sequence space, inside the promise) so that len == 2^30 exactly, which the issue asks
      for in the same breath and which is the case that showed a build-then-refuse bug on the capture-order path.  The expectation is
      stream_seq_model.build_np (lexsort, running maximum); the arena is compared by reshape against one period (2 570 payloads) of kept
      bytes assembled from the period's payloads through segs.
tests/test_streams_seq_high_model.py holds tiled, build_np, the schedule's closed forms and the device layout to stream_seq_model.build
on three periods and a rest, without a GPU.

Address arithmetic read before the first run, for offsets, sums and destinations of 2^32 and more (csrc/kmp_streams_seq.hip):
    kmp_sseq_heads_kernel, kmp_sseq_keys_kernel   i, s uint64; head_pos and val are positions and payload numbers below 2^32 (n < 2^32).
                     key2 = key << 32 | lo with key = flow << 1 | dir below 2^32.  No byte offset.  Clean.
    kmp_sseq_max_scan_kernel / _totals   v = s << 33 | (uint64)off + L: off < 2^32 and L <= 2^30, so end < 2^33 and the stream above it
                     (s < 2^31: below 2^64).  Clean.
    kmp_sseq_take_scan_kernel    `to` uint64 (masked to 33 bits), ahead = (int64)to - (int64)off, one signed 64-bit difference; take and
                     skip 32-bit (<= L); tb, b[], s_b[], eb, tsum[], blk_tsum[] all uint64; the gap counts 32-bit (< n).  Clean.
    kmp_sseq_take_totals_kernel  cb uint64, blk_tsum[i] = cb + s_b - vb0 in 64 bits, grand[1] uint64.  Clean.
    kmp_sseq_records_kernel      members, bytes uint64 differences of sum_at (64-bit); len = (uint32)min(bytes, depth) <= 2^30;
                     gap_bytes = last - bytes and dup_bytes = members - bytes in 64 bits into 64-bit record words.  Clean.
    kmp_sseq_index_kernel        pkt_off[s] = blk_bytes[..] + loc_off[s] uint64; pos a difference of 64-bit sums, written as two halves;
                     at = (uint32)min(pos, len) <= 2^30; piece_dst = uint64 + at; the piece's source address as two halves of so.  Clean.
    kmp_sseq_gather_kernel       u, u0, span, u_end uint64; d = u * 16u with u uint64; advance_piece over uint64 keys with q uint64 and a
                     32-bit piece number; d - pd < 2^30 where the piece holds the byte, pd - d < 16 otherwise (start >= -15);
                     dst + u * 16u in 64 bits.  Clean.
    kmpgpu.hip       the arena of the streams is sized from the 64-bit total of kmp_scan_totals_kernel; kmp_validate_index_kernel takes
                     len up to 2^30 (the sibling's fix).  Clean.
    matcher.py       stream_locate_ordered: stream << 31 | pos for pos < 2^31 only, uint64.  Clean.
Nothing wrong was found by reading, and no byte or record came out wrong in the runs: csrc/ is unchanged.

What the runs showed beside that (one run's figures, printed by the tests, asserted nowhere): behind an odd cut the ordered gather searches
past the 0-byte pieces that kmp_stream_gather_kernel walks.  One stream of 800 000 members of 1 458 bytes with 100 000 behind the cut:
kmpgpu_load_streams_ordered kernel_ms 1.204 at depth 1 020 599 993 and 1.163 at 1 020 599 984; kmpgpu_load_streams 21.974 and 0.943 in
the same process.

Memory.  By the sizes, not measured.  Device: the source 4.72 GB (test_ordered_streams_past_2_32) or 4.56 GB (the long source of the
other two, laid out once per test), dst 4.51 GB and 4.43 GB (1 GiB in the other two) plus an eighth of headroom, the sort buffers, scans,
pieces, map and segs of 6.25 M payloads below 1.5 GB: a peak of about 11.5 GB in test_ordered_streams_past_2_32, 6.5 GB in the others.
Host: one download of up to 4.51 GB at a time beside about 0.7 GB of expected records; each test is skipped where MemAvailable is under
twice its download -- the module's only skip.

Run on a real MI355X:  python -m pytest tests/test_gpu_streams_seq_high.py -m gpu
Measured there (call times of one run; tests/test_gpu_high_destinations.py in the same run beside them): test_ordered_streams_past_2_32 9.0 s (destinations of 4.51
and 4.43 GB; the ordered call's kernel_ms 13.6 and 5.3), test_long_udp_stream_through_the_ordered_call 7.4 s,
test_long_tcp_stream_to_the_depth 2.1 s (kernel_ms 1.31 and 1.25); the sibling's test_streams_past_2_32 10.6 s, test_selected_past_2_32
10.1 s, test_stream_longer_than_2_32 7.6 s, test_decoded_past_2_32 7.5 s.

Checked to bite: memory-safe changes to scratch builds (never committed), each run once over this module and
tests/test_gpu_streams_seq_span.py.  Every wrong address lies inside the same allocation and every source read stays inside its member;
none cuts piece_dst, the pieces' source address, tsum / blk_tsum or a loop bound.
  1   kmp_sseq_gather_kernel, dst + (uint32_t)(u * 16u)           test_ordered_streams_past_2_32: 20 466 260 bytes of periods 0 .. 127 differ,
                                                                  from byte 0
  2   kmp_sseq_index_kernel, pkt_off[s] cut to 32 bits            test_ordered_streams_past_2_32: 535 026 bytes of periods 23 040 .. 23 167 differ,
                                                                  the first at 4 294 976 320 (the library repacks the overlapping slots, so off passes)
  3   kmp_sseq_index_kernel, high word of pos written as 0        test_long_udp_stream_through_the_ordered_call: the map differs from member
                                                                  2 945 794 on
  4   kmp_sseq_records_kernel, bytes cut to 32 bits               test_long_udp_stream_through_the_ordered_call: record 0 differs
  5   kmp_sseq_take_scan_kernel, ahead = (int32_t)((uint32_t)to - M.off)     nothing fails, here or in tests/test_gpu_streams_seq_span.py:
                                                                  the change is no fault -- `ahead` lies in [-2^31, 2^30] for every input
                                                                  (that module's docstring has the argument)
  5b  the running maximum packed as stream << 30 | end            all 10 tests of tests/test_gpu_streams_seq_span.py fail (run over that module,
                                                                  test_gpu_streams_seq.py and test_gpu_streams_seq_scale.py, whose 34 tests pass)
Every other test of the two modules passed on each of builds 1 to 5.  A build with changes 1 to 5 at once was run once over
tests/test_gpu_streams_seq.py and tests/test_gpu_streams_seq_scale.py: 34 passed -- the gap this module closes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import (B32, FLOW_A, FLOW_B, PERIOD, check_periodic_bytes, meta_of_flows, reset, tag_counts, tagged, torch)  # noqa: E402  (torch first)

import prep_model as PM  # noqa: E402
import stream_model as TM  # noqa: E402
import stream_seq_model as QM  # noqa: E402
from multithreading_string_matching_amd.matcher import KERNEL_GENERAL, OPT_NONTEMPORAL, stream_locate_ordered  # noqa: E402
from test_gpu_high_destinations import (BEHIND, FAMILIES, HIGH, LONG_TAGS, MEMBER, N_LONG, N_SHORT, REST, TAGS, Destination,  # noqa: E402,F401
                                        LongStream, check_stream_records, check_tags, cut_to, filler, host_can_hold, period_lens, source,
                                        stream_period)
from test_gpu_prep_scale import _scan  # noqa: E402

FULL = 1 << 30
PERIOD_FLOWS = 6
SEQ_MASK = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------
# 1. the periodic capture: numpy, no device (tests/test_streams_seq_high_model.py holds it to the plain model)
# ------------------------------------------------------------------------------------------------
def segment_offsets(rng, lens):
    """sequence offsets for segments of the given lengths in sending order, the shape of test_gpu_streams_seq._segments: 8 % start where
    an earlier one started (covered wholly or in front), 12 % start 1 .. 40 bytes in front of what was sent so far, 5 % behind a hole of
    1 .. 29 bytes"""
    offs, at = [], 0
    for L in lens:
        r = rng.random()
        if offs and r < 0.08:
            o = offs[int(rng.integers(len(offs)))]
        elif at > 0 and r < 0.2:
            o = at - min(at, int(rng.integers(1, 41)))
        else:
            o = at + (int(rng.integers(1, 30)) if r > 0.95 else 0)
        offs.append(o)
        at = max(at, o + int(L))
    return offs


def ordered_period(seed=2035):
    """(pay, meta, seq) of one period: the sibling's stream_period in 6 flows, both directions, flow 4 UDP; every stream's segments handed
    to its members in a random order under an ISN of its own, every third one within 500 of 2^32"""
    pay = stream_period()
    rng = np.random.default_rng(seed)
    e = np.arange(PERIOD)
    flow = (e // 2) % PERIOD_FLOWS                                 # a long and a short payload in turn: streams of about equal sizes
    back = (e // (2 * PERIOD_FLOWS)) % 3 == 2                      # every third round the answers: direction 0 is the forward one
    meta = meta_of_flows(flow, seed=seed)
    meta["src_ip"], meta["dst_ip"] = np.where(back, FLOW_B, FLOW_A + flow), np.where(back, FLOW_A + flow, FLOW_B)
    meta["src_port"], meta["dst_port"] = np.where(back, 53, 1000 + flow), np.where(back, 1000 + flow, 53)
    meta["proto"] = np.where(flow == 4, 17, 6)
    seq = np.zeros(PERIOD, dtype=np.uint32)
    for s, (f, d, ks) in enumerate(TM.members(meta)):
        isn = (1 << 32) - int(rng.integers(1, 500)) if s % 3 == 0 else int(rng.integers(1, 1 << 32))
        sent = rng.permutation(ks)
        for k, o in zip(sent, segment_offsets(rng, [len(pay[k]) for k in sent])):
            seq[k] = (isn + o) & SEQ_MASK
    seq[seq == 0] = 1                                              # (a UDP member's is arbitrary and nonzero)
    return pay, meta, seq


def capture_meta(meta, reps, rest):
    """the metadata of `reps` periods and the first `rest` payloads of one more: period r between flows of its own, the address that is
    not FLOW_B moved on by r << 3"""
    P = len(meta)
    big = np.concatenate([np.tile(meta, reps), meta[:rest]])
    r = (np.arange(len(big), dtype=np.uint32) // np.uint32(P)) << np.uint32(3)
    for field in ("src_ip", "dst_ip"):
        big[field] = np.where(big[field] == FLOW_B, big[field], big[field] + r)
    return big


def capture_seq(seq, reps, rest, device="cuda"):
    """the sequence numbers of the same capture as a tensor of 32-bit integers on `device`, tiled there"""
    one = torch.from_numpy(np.ascontiguousarray(seq).view(np.int32)).to(device)
    return torch.cat([one.repeat(reps), one[:rest]]).contiguous()


def tiled(model, rest_model, P, reps, depth):
    """What dst has to hold of `reps` periods and a rest, from the model of one period and the model of the rest (both built at the full
    depth): records and map with their indices moved on, segs and orders tiled, index, the arena as `per` x `reps` + `head`, the tag
    counts."""
    out = {"reps": reps}
    parts = []
    for (streams, recs, pos, segs, orders, _), times in ((model, reps), (rest_model, 1)):
        S, F = len(recs), int(recs["flow"].max()) + 1
        recs = cut_to(recs, depth)
        parts.append((S, F, [s[:depth] for s in streams], np.tile(recs, times), np.tile(pos, times), np.tile(segs, times), np.tile(orders, times)))
    (S, F, streams, recs, pos, segs, orders), (S1, _, streams1, recs1, pos1, segs1, orders1) = parts
    rs = np.concatenate([np.repeat(np.arange(reps), S), np.full(S1, reps)]).astype(np.uint64)
    rp = np.concatenate([np.repeat(np.arange(reps), P), np.full(len(pos1), reps)]).astype(np.uint64)
    out["recs"], out["pos"] = np.concatenate([recs, recs1]), np.concatenate([pos, pos1])
    out["segs"], out["orders"] = np.concatenate([segs, segs1]), np.concatenate([orders, orders1])
    out["recs"]["first_packet"] += rs * np.uint64(P)
    out["recs"]["last_packet"] += rs * np.uint64(P)
    out["recs"]["flow"] += (rs * np.uint64(F)).astype(np.uint32)
    out["pos"]["stream"] += (rp * np.uint64(S)).astype(np.uint32)
    per, poff, pln = TM.arena(streams)
    head, hoff, hln = TM.arena(streams1)
    pb = len(per)
    out["per"], out["head"], out["end"] = per, head, reps * pb + len(head)
    r = np.arange(reps, dtype=np.uint64)[:, None]
    out["off"] = np.concatenate([(r * np.uint64(pb) + poff[None, :]).ravel(), np.uint64(reps * pb) + hoff]).astype(np.uint64)
    out["len"] = np.concatenate([np.tile(pln, reps), hln]).astype(np.uint32)
    out["tags"] = tag_counts(streams, [reps] * S) + tag_counts(streams1, [1] * S1)
    out["n_flows"] = (reps + 1) * F
    return out


def forward_cut(model):
    """a depth that is no multiple of 16 and shortens every forward stream of the period"""
    recs = model[1]
    cut = int(recs["bytes"][recs["dir"] == 0].min()) - 5
    return cut - 1 if cut % 16 == 0 else cut


# ------------------------------------------------------------------------------------------------
# 3. the schedule of test_long_tcp_stream_to_the_depth
# ------------------------------------------------------------------------------------------------
N_TCP = 830_000
GROUP = 10
ISN = 0xFFFFF000


def schedule(L):
    """(sequence offsets of the ten payloads of a group from the group's start, the group's size in sequence space, the kept
    (payload, skip, take) of a group in stream order): 3 bytes of hole, then 0 1 2 3 back to back, 4 = 3 once more, 5 6, 7 from 100 bytes
    before the end of 6, then what capture order has as 9 and 8"""
    assert L > 100
    offs = np.array([3, 3 + L, 3 + 2 * L, 3 + 3 * L, 3 + 3 * L, 3 + 4 * L, 3 + 5 * L, 3 + 6 * L - 100, 3 + 8 * L - 100, 3 + 7 * L - 100], dtype=np.int64)
    kept = [(0, 0, L), (1, 0, L), (2, 0, L), (3, 0, L), (5, 0, L), (6, 0, L), (7, 100, L - 100), (9, 0, L), (8, 0, L)]
    return offs, 3 + 9 * L - 100, kept


def scheduled_seq(n, L, isn=ISN):
    offs, size, _ = schedule(L)
    k = np.arange(n, dtype=np.int64)
    return ((isn + (k // GROUP) * size + offs[k % GROUP] - 3) & SEQ_MASK).astype(np.uint32)       # the stream's offset 0 is payload 0


def scheduled_tallies(n, L):
    """(bytes, n_gaps, gap_bytes, dup_bytes) of the stream of n payloads, n a multiple of 10, in closed form"""
    assert n % GROUP == 0
    g = n // GROUP
    return g * (9 * L - 100), g - 1, 3 * (g - 1), g * (L + 100)


def scheduled_locate(x, L):
    """(payload, offset in it) of byte x of the stream, in closed form"""
    _, _, kept = schedule(L)
    g, r = divmod(int(x), 9 * L - 100)
    for i, skip, take in kept:
        if r < take:
            return g * GROUP + i, skip + r
        r -= take
    raise AssertionError


def kept_period(pay, segs, pos, n):
    """the stream's bytes of the first n payloads (one period of everything: n = lcm(257, 10)), from the period's payloads through segs"""
    order = np.argsort(pos["pos"][:n], kind="stable")
    order = order[segs["take"][order] > 0]
    assert (np.diff(pos["pos"][order].astype(np.int64)) == segs["take"][order][:-1]).all()
    return np.frombuffer(b"".join(pay[int(k) % PERIOD][int(segs["skip"][k]):int(segs["skip"][k]) + int(segs["take"][k])] for k in order), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# the device side
# ------------------------------------------------------------------------------------------------
def check_ordered_records(dst, want, meta):
    check_stream_records(dst, want["recs"], want["pos"], meta)
    gsegs, gorders = dst.stream_segs(), dst.stream_orders()
    assert gsegs.tobytes() == want["segs"].tobytes(), np.flatnonzero(gsegs != want["segs"])[:4]
    assert gorders.tobytes() == want["orders"].tobytes(), np.flatnonzero(gorders != want["orders"])[:4]


def test_ordered_streams_past_2_32(source):
    pay, pmeta, pseq = ordered_period()
    model, rest_model = QM.build(pay, pmeta, pseq, FULL), QM.build(pay[:REST], pmeta[:REST], pseq[:REST], FULL)
    recs, segs, orders = model[1], model[3], model[4]
    cut = forward_cut(model)
    assert len(recs) == len(rest_model[1]) == 2 * PERIOD_FLOWS and 0 < (orders["tcp"] == 0).sum() < len(recs)
    assert cut % 16 and (recs["bytes"][recs["dir"] == 0] > cut).all() and (rest_model[1]["bytes"] < cut).any()
    assert ((segs["skip"] > 0) & (segs["take"] > 0)).sum() > 15 and ((segs["take"] == 0) & (segs["skip"] > 0)).sum() > 10
    assert orders["n_gaps"].sum() > 5 and (segs["skip"][::2] >= 8).sum() > 10          # covered fronts that hold a tag
    per_cut = len(TM.arena([s[:cut] for s in model[0]])[0])
    reps = -(-(HIGH + (1 << 20)) // per_cut)
    n = reps * PERIOD + REST
    host_can_hold(reps * len(TM.arena(model[0])[0]) + (1 << 20))
    meta = capture_meta(pmeta, reps, REST)
    src = source.build(pay, n)
    src.set_meta(meta)
    d_seq = capture_seq(pseq, reps, REST)
    torch.cuda.synchronize()
    assert src.build_flows() == (reps + 1) * PERIOD_FLOWS
    print(f"kmpgpu_load_streams_ordered over {n} payloads in {reps} periods and a rest of {REST}, {(reps + 1) * PERIOD_FLOWS} flows")
    with Destination() as dst:
        for depth, nontemporal in ((FULL, 1), (cut, 0)):
            want = tiled(model, rest_model, PERIOD, reps, depth)
            assert want["end"] > HIGH and B32 % len(want["per"]) != 0 and want["n_flows"] == (reps + 1) * PERIOD_FLOWS
            assert (depth == cut) == bool((want["recs"]["bytes"] > want["recs"]["len"]).any())
            dst.set_option(OPT_NONTEMPORAL, nontemporal)
            assert dst.load_streams(src, depth, seq=d_seq) == len(want["recs"])
            print(f"    depth {depth}: destination of {want['end']} bytes, kernel_ms {dst.last_timing().kernel_ms:.3f}")
            check_ordered_records(dst, want, meta)
            assert dst.arena_info() == (len(want["recs"]), int(want["recs"]["len"].sum(dtype=np.uint64)))
            a, off, ln = dst.arena_download()
            assert np.array_equal(off, want["off"]), np.flatnonzero(off != want["off"])[:4]
            assert np.array_equal(ln, want["len"]) and np.array_equal(ln, want["recs"]["len"])
            check_periodic_bytes(a, want)
            del a
            assert (want["tags"] >= reps).sum() > 150 and want["tags"].sum() < n - reps * int((segs["take"] == 0).sum())
            check_tags(dst, want["tags"])
    del d_seq
    source.release()


def run_long(long, dst, n, depth, seq, want=None):
    """LongStream.run through the ordered call: load_streams(seq=...) of the first n payloads of the long source as one stream; records,
    map, segs, orders, index and every byte.  want: (recs, pos, segs, orders, one period of the stream's bytes); None: what
    kmpgpu_load_streams gives, with nothing dropped.  Returns (the map, kernel_ms)."""
    meta, lens = np.repeat(long.one, n), period_lens(long.pay, n)
    m = long.source.use(n)
    m.set_meta(meta)
    assert m.build_flows() == 1
    if want is None:
        recs, pos = TM.records_np(meta, lens, depth)
        segs, orders = np.zeros(n, dtype=QM.SEG_DTYPE), np.zeros(1, dtype=QM.ORDER_DTYPE)
        segs["take"] = lens
        whole = long.whole
    else:
        recs, pos, segs, orders, whole = want
    assert dst.load_streams(m, depth, seq=seq[:n]) == 1
    ms = dst.last_timing().kernel_ms
    check_ordered_records(dst, {"recs": recs, "pos": pos, "segs": segs, "orders": orders}, meta)
    assert recs["len"].tolist() == [depth] and recs["n_packets"].tolist() == [n] and dst.arena_info() == (1, depth)
    a, off, ln = dst.arena_download()
    assert off.tolist() == [0] and ln.tolist() == [depth]
    assert len(a) == (depth + 15) // 16 * 16 + 64 and not a[depth:].any()
    reps = depth // len(whole)
    body = a[:reps * len(whole)].reshape(reps, len(whole))
    for lo in range(0, reps, 64):
        assert (body[lo:lo + 64] == whole).all(), (lo, np.argwhere(body[lo:lo + 64] != whole)[0].tolist())
    assert np.array_equal(a[reps * len(whole):depth], whole[:depth - reps * len(whole)])
    return dst.stream_map(), ms


def test_long_udp_stream_through_the_ordered_call(source):
    long = LongStream(source)
    assert int(long.one["proto"][0]) == 17
    seq = (torch.arange(N_LONG, dtype=torch.int64, device="cuda") * 2654435761 % (1 << 31) + 1).to(torch.int32)      # arbitrary, nonzero
    torch.cuda.synchronize()
    with Destination([TAGS[t] for t in LONG_TAGS]) as dst:
        depth = FULL
        gmap, _ = run_long(long, dst, N_LONG, depth, seq)
        assert int(dst.streams()["bytes"][0]) == N_LONG * MEMBER > HIGH
        long.check_high_words(gmap, depth)
        orders, segs = dst.stream_orders(), dst.stream_segs()
        assert orders.tobytes() == bytes(len(orders) * orders.itemsize) and len(orders) == 1
        assert not segs["skip"].any() and (segs["take"] == MEMBER).all() and not segs["seq_off"].any() and not segs["reserved"].any()
        behind = int((gmap["pos"].astype(np.int64) + 8 <= depth).sum())
        want = [(behind - t + PERIOD - 1) // PERIOD for t in LONG_TAGS]
        assert behind == (depth - 8) // MEMBER + 1 and sum(want) > 8000
        for kernel in FAMILIES + (KERNEL_GENERAL,):
            assert _scan(dst, kernel).tolist() == want, kernel
        reset(dst)
        odd = (N_SHORT - BEHIND) * MEMBER - 7
        assert odd % 16 and odd < FULL
        for depth in (odd, odd // 16 * 16):
            _, ms = run_long(long, dst, N_SHORT, depth, seq)
            dst.load_streams(long.source.m, depth)
            plain = dst.last_timing().kernel_ms
            print(f"one stream of {N_SHORT} members of {MEMBER} bytes, depth {depth} (% 16 = {depth % 16}), {BEHIND} members behind the cut: "
                  f"kmpgpu_load_streams_ordered kernel_ms {ms:.3f}, kmpgpu_load_streams kernel_ms {plain:.3f}")
    del seq
    source.release()


def test_long_tcp_stream_to_the_depth(source):
    long = LongStream(source)                                       # (lays out 3.1 M payloads; this test borrows the first 830 000)
    long.one["proto"] = 6
    n, L = N_TCP, MEMBER
    lens = period_lens(long.pay, n)
    assert (lens == L).all() and n % GROUP == 0
    h_seq = scheduled_seq(n, L)
    assert int(h_seq[0]) > int(h_seq[-1])                           # the sequence numbers wrap
    seq = torch.from_numpy(h_seq.view(np.int32)).cuda()
    torch.cuda.synchronize()
    meta = np.repeat(long.one, n)
    uncut = QM.build_np(lens, meta, h_seq, FULL)
    kept, gaps, gap_bytes, dup_bytes = scheduled_tallies(n, L)
    o = uncut[3][0]
    assert (int(uncut[0]["bytes"][0]), int(o["n_gaps"]), int(o["gap_bytes"]), int(o["dup_bytes"]), int(o["tcp"]), int(o["seq_base"])) == \
        (kept, gaps, gap_bytes, dup_bytes, 1, ISN)
    assert kept > FULL and (n // GROUP) * schedule(L)[1] < 1 << 31  # reaches the depth; spans less than 2^31 of sequence space
    whole = kept_period(long.pay, uncut[2], uncut[1], PERIOD * GROUP)
    assert len(whole) == PERIOD * (9 * L - 100) == int(uncut[1]["pos"][PERIOD * GROUP])
    odd = FULL - 12345
    assert odd % 16
    with Destination([TAGS[t] for t in LONG_TAGS]) as dst:
        for depth in (FULL, odd):
            recs, pos, segs, orders = QM.build_np(lens, meta, h_seq, depth)
            assert recs["len"].tolist() == [depth] and pos.tobytes() == uncut[1].tobytes()
            gmap, ms = run_long(long, dst, n, depth, seq, (recs, pos, segs, orders, whole))
            print(f"one TCP stream of {n} members on the schedule, depth {depth}: kernel_ms {ms:.3f}")
            gsegs = dst.stream_segs()
            got = dst.stream_orders()[0]
            assert (int(got["n_gaps"]), int(got["gap_bytes"]), int(got["dup_bytes"])) == (gaps, gap_bytes, dup_bytes)
            g = (odd // (9 * L - 100) - 3) * (9 * L - 100)          # a group in front of both cuts
            at = np.array([0, odd - 1, odd, FULL - 1, g + 4 * L - 1, g + 4 * L, g + 6 * L + (L - 100) - 1, g + 6 * L + (L - 100)], dtype=np.uint64)
            k, j = stream_locate_ordered(gmap, gsegs, np.zeros(len(at), dtype=np.uint64), at)
            assert list(zip(k.tolist(), j.tolist())) == [scheduled_locate(x, L) for x in at]
            assert k[4] % GROUP == 3 and k[5] % GROUP == 5 and j[5] == 0          # on both sides of the covered member 4
    del seq
    source.release()
