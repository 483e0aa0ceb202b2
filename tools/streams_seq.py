"""What flow streams by TCP sequence number cost (profiles/streams_seq.txt).

    python3 tools/streams_seq.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 20] [--depth 1073741824] [--scan-depth 1048576] [--out profiles/streams_seq.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the calls alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.  The metadata is that of tools/flows.py (every flow TCP), for its three shapes: ONE flow,
10 000 flows with Zipf sizes, every payload its own flow.
  (1) unchanged paths  kmpgpu_scan_rules (strings.txt's 97 tokens and 100 generated rules), kmpgpu_load_seams and kmpgpu_load_streams: the
                       parent commit's library (--parent-lib; left out without it) against this tree's, by turns.  The outputs must be
                       equal; the criterion is this tree's median inside the parent's own min .. max of the run.
  (2) in order         kmpgpu_load_streams_ordered with sequence numbers that agree with capture order, against kmpgpu_load_streams in
                       the same rounds, kernel by kernel from kmpgpu_profile_begin.  The two gathers move the same pieces: the yardstick
                       for the new one is the capture-order gather's own min .. max.  The records and the map must be equal.
  (3) retransmissions  the same with one payload in ten an exact retransmission of the segment before it in its stream.
  (4) scan_flows       kmpgpu_scan_flows(rules, scope flow) on the ordered streams cut to --scan-depth against the capture-order ones."""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

from flows import gen_flows, gen_meta  # noqa: E402  (tools/flows.py: the same shapes)
from headers import gen_rules, matcher_on, spread, timed  # noqa: E402  (tools/headers.py: the same instrument)

CAPTURE = ("keys", "sort", "stream scan + totals", "heads + records + slot scan x 2", "index", "gather")
ORDERED = ("keys", "sort", "stream scan + totals", "heads + keys 2 + sort 2", "max scan + totals + take scan + totals",
           "records + slot scan x 2", "index", "gather")


def sequence_numbers(smap, L, dup=None, seed=9):
    """seq[k] for members of L bytes each: every stream starts at a number of its own (some just below 2^32) and goes on in capture
    order; with dup (bool per payload, never a stream's first member) a marked payload repeats the segment sent before it"""
    n = len(smap)
    rng = np.random.default_rng(seed)
    stream = smap["stream"].astype(np.int64)
    isn = rng.integers(0, 1 << 32, int(stream.max()) + 1, dtype=np.uint64)
    isn[::3] = (1 << 32) - 1 - rng.integers(0, 500, len(isn[::3]), dtype=np.uint64)
    if dup is None:
        off = smap["pos"]
    else:
        order = np.argsort(stream, kind="stable")
        new = (~dup[order]).astype(np.int64)
        before = np.cumsum(new) - new                           # new segments in front of the member, over all streams
        head = np.ones(n, dtype=bool)
        head[1:] = stream[order][1:] != stream[order][:-1]
        before -= before[np.flatnonzero(head)][np.cumsum(head) - 1]
        off = np.zeros(n, dtype=np.uint64)
        off[order] = ((before - dup[order]) * L).astype(np.uint64)
    return ((isn[stream] + off) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--depth", type=int, default=1 << 30)
    ap.add_argument("--scan-depth", type=int, default=1 << 20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_seq.txt"))
    args = ap.parse_args()
    n, L, stride, depth = args.payloads, 1500, 1504, args.depth
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"flow streams by sequence number (kmpgpu_load_streams_ordered), {n} x {L} B, depth {depth}, medians of {args.reps} rounds with "
             f"min / quartiles / max, ms (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    ms = {"b": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    st, sq = GpuMatcher(0), GpuMatcher(0)                         # capture order, sequence order
    others = {key: (matcher_on(args.parent_lib) if key == "a" else GpuMatcher(0)) for key in ms}      # dst of the unchanged loaders
    everyone = list(ms.values()) + [st, sq] + list(others.values())
    try:
        for m in everyone:
            m.set_stream(stream.cuda_stream)
        b = ms["b"]
        b.fixed_index(d_off, d_len, L, 16)
        b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=b"NEEDLE_16B_PATRN", plant_permille=100))
        b.sync()
        rules = gen_rules(random.Random(100), 100, len(tokens))
        for m in ms.values():
            m.set_patterns(tokens)
            m.attach_arena(d_arena, d_off, d_len)
            m.set_rules(rules)
        for m in [st, sq] + list(others.values()):
            m.set_patterns(tokens)
        st.set_rules(rules)
        sq.set_rules(rules)

        def by_turns(label, calls, check=None):
            """calls: {key: function}; check(results): what must hold between them"""
            if check:
                check({key: fn() for key, fn in calls.items()})
            t = {key: [] for key in calls}
            for rnd in range(3 + args.reps):
                for key, fn in calls.items():
                    dt, _ = timed(stream, fn)
                    if rnd >= 3:
                        t[key].append(dt)
            line = f"{label}: " + "; ".join(f"({key}) {spread(v)}" for key, v in t.items())
            if "a" in t and "b" in t:
                mb = statistics.median(t["b"])
                line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
            say(line)
            return t

        def same_rules(res):
            if "a" in res:
                for k in ("hits", "any", "counts"):
                    assert np.array_equal(res["a"][k], res["b"][k]), k

        def medians(kk, names):
            return [statistics.median([k[i] for k in kk]) for i in range(len(names))]

        def parts(kk, names):
            return ", ".join(f"{nm} {v:.3f}" for nm, v in zip(names, medians(kk, names)))

        by_turns(f"(1) kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules, (a) parent (b) this tree",
                 {key: (lambda m=m: m.scan_rules(hits=True)) for key, m in ms.items()}, same_rules)
        for shape in ("one flow", "10 000 flows, Zipf sizes", "every payload its own flow"):
            flow = gen_flows(shape, n)
            meta = gen_meta(flow)
            d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1).copy()).cuda()
            for m in ms.values():
                m.set_meta(d_meta)
                assert m.build_flows() == int(flow.max()) + 1
            # ---- (1) the unchanged loaders
            def same_seams(res):
                if "a" in res:
                    assert res["a"] == res["b"] and others["a"].seams().tobytes() == others["b"].seams().tobytes()

            def same_streams(res):
                if "a" in res:
                    assert res["a"] == res["b"] and others["a"].streams().tobytes() == others["b"].streams().tobytes()
                    assert others["a"].stream_map().tobytes() == others["b"].stream_map().tobytes()
            by_turns(f"(1) {shape}, kmpgpu_load_seams(reach 98), (a) parent (b) this tree",
                     {key: (lambda key=key: others[key].load_seams(ms[key], 98)) for key in ms}, same_seams)
            by_turns(f"(1) {shape}, kmpgpu_load_streams(depth {depth}), (a) parent (b) this tree",
                     {key: (lambda key=key: others[key].load_streams(ms[key], depth)) for key in ms}, same_streams)
            # ---- (2) in order: the new call against the capture-order one, kernel by kernel, in the same rounds
            n_streams = st.load_streams(b, depth)
            smap = st.stream_map()
            seq = sequence_numbers(smap, L)
            d_seq = torch.from_numpy(seq.view(np.int32)).cuda()
            assert sq.load_streams(b, depth, seq=d_seq) == n_streams
            assert sq.streams().tobytes() == st.streams().tobytes() and sq.stream_map().tobytes() == smap.tobytes(), "in order: the two calls disagree"
            orders = sq.stream_orders()
            assert orders["tcp"].all() and not orders["dup_bytes"].any() and not orders["n_gaps"].any()

            def rounds(d_seq):
                tc, kc, to, ko = [], [], [], []
                for rnd in range(3 + args.reps):
                    st.profile_begin(16)
                    st.load_streams(b, depth)
                    pc = st.profile_end(16)
                    sq.profile_begin(16)
                    sq.load_streams(b, depth, seq=d_seq)
                    po = sq.profile_end(16)
                    if rnd >= 3:
                        tc.append(st.last_timing().kernel_ms); kc.append(pc)
                        to.append(sq.last_timing().kernel_ms); ko.append(po)
                assert all(len(k) == len(CAPTURE) for k in kc) and all(len(k) == len(ORDERED) for k in ko), (len(kc[0]), len(ko[0]))
                return tc, kc, to, ko

            tc, kc, to, ko = rounds(d_seq)
            gc, go = [k[-1] for k in kc], [k[-1] for k in ko]
            inside = min(gc) <= statistics.median(go) <= max(gc)
            nbytes = sq.arena_info()[1]
            extra = sum(medians(ko, ORDERED)[3:5])
            say(f"(2) {shape}, in order ({n_streams} streams, {nbytes} bytes; kernel_ms of kmpgpu_last_timing): (capture) kmpgpu_load_streams {spread(tc)}; "
                f"kernels: {parts(kc, CAPTURE)}; (seq) kmpgpu_load_streams_ordered {spread(to)}; kernels: {parts(ko, ORDERED)}; "
                f"gather (capture) {spread(gc)}; gather (seq) {spread(go)}; (seq) / (capture) {statistics.median(go) / statistics.median(gc):.4f}; "
                f"(seq)'s median inside (capture)'s range: {'yes' if inside else 'NO'}; the gather moves 2 x {nbytes} bytes at "
                f"{2 * nbytes / statistics.median(go) / 1e6:.0f} GB/s; second order + scans {extra:.3f}; sum of the parts "
                f"{sum(medians(ko, ORDERED)):.3f} against the whole {statistics.median(to):.3f}; whole (seq) - whole (capture) "
                f"{statistics.median(to) - statistics.median(tc):.3f}")
            # ---- (3) one payload in ten retransmits the segment before it
            rng = np.random.default_rng(17)
            dup = (rng.random(n) < 0.1) & (smap["pos"] > 0)
            d_dup = torch.from_numpy(sequence_numbers(smap, L, dup).view(np.int32)).cuda()
            assert sq.load_streams(b, depth, seq=d_dup) == n_streams
            orders, segs = sq.stream_orders(), sq.stream_segs()
            assert int(orders["dup_bytes"].sum()) == int(dup.sum()) * L and not orders["n_gaps"].any(), "retransmissions: dup_bytes"
            assert np.array_equal(segs["take"] == 0, dup) and sq.arena_info()[1] == (n - int(dup.sum())) * L
            tc, kc, to, ko = rounds(d_dup)
            kept = sq.arena_info()[1]
            say(f"(3) {shape}, {int(dup.sum())} exact retransmissions ({kept} bytes kept): (seq) kmpgpu_load_streams_ordered {spread(to)}; kernels: "
                f"{parts(ko, ORDERED)}; the gather moves 2 x {kept} bytes at {2 * kept / statistics.median([k[-1] for k in ko]) / 1e6:.0f} GB/s; "
                f"(capture) kmpgpu_load_streams in the same rounds {spread(tc)}")
            # ---- (4) the flow verdict on the ordered streams
            st.load_streams(b, args.scan_depth)
            sq.load_streams(b, args.scan_depth, seq=d_seq)
            for m in (st, sq):
                assert m.build_flows() == int(flow.max()) + 1

            def same_verdict(res):
                assert np.array_equal(res["seq"]["flow_counts"], res["capture"]["flow_counts"])
            by_turns(f"(4) {shape}, depth {args.scan_depth} ({sq.arena_info()[1]} bytes), kmpgpu_scan_flows(rules, scope flow) on the streams in "
                     f"(seq) sequence order, (capture) capture order, (b) on src",
                     {"seq": lambda: sq.scan_flows("rules", "flow"), "capture": lambda: st.scan_flows("rules", "flow"),
                      "b": lambda: b.scan_flows("rules", "flow")}, same_verdict)
        by_turns("(1) kmpgpu_scan_rules after the stream calls, (a) parent (b) this tree",
                 {key: (lambda m=m: m.scan_rules(hits=True)) for key, m in ms.items()}, same_rules)
    finally:
        for m in everyone:
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
