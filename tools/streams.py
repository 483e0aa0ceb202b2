"""What flow streams cost (profiles/streams.txt).

    python3 tools/streams.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 20] [--depth 1073741824] [--scan-depth 1048576] [--out profiles/streams.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the calls alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.  The metadata is that of tools/flows.py, for its three shapes: ONE flow, 10 000 flows with
Zipf sizes, every payload its own flow.
  (1) unchanged paths  kmpgpu_scan_rules (strings.txt's 97 tokens and 100 generated rules) and kmpgpu_load_seams: the parent commit's
                       library (--parent-lib; left out without it) against this tree's.  The outputs must be equal.
  (2) load_streams     kmpgpu_load_streams per shape and its kernels from kmpgpu_profile_begin (keys, sort, stream scan + totals,
                       heads + records + the two slot scan kernels, index, gather); the records and the map are checked against numpy.
                       In the same rounds kmpgpu_load_selected with all bits set -- the same bytes read and written once: the yardstick
                       for the gather -- and kmpgpu_load_seams.
  (3) scan_flows       kmpgpu_scan_flows(rules, scope flow) on the stream context, its streams cut to --scan-depth (a payload is scanned
                       by one wavefront: the depth bounds the longest serial piece of the pass), against kmpgpu_scan_flows_seams on src."""
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
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import STREAM_DTYPE, STREAM_POS_DTYPE, GpuMatcher  # noqa: E402

from flows import gen_flows, gen_meta  # noqa: E402  (tools/flows.py: the same shapes)
from headers import gen_rules, matcher_on, spread, timed  # noqa: E402  (tools/headers.py: the same instrument)


def host_streams(meta, fo, first_meta, depth, L):
    """the stream records and the map with numpy: a stable sort by (flow, dir) keeps capture order; every payload is L bytes"""
    f1 = first_meta[fo]
    dr = ~((meta["src_ip"] == f1["src_ip"]) & (meta["src_port"] == f1["src_port"]) & (meta["dst_ip"] == f1["dst_ip"])
           & (meta["dst_port"] == f1["dst_port"]))
    key = fo.astype(np.uint64) << np.uint64(1) | dr.astype(np.uint64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(fo), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    hp = np.flatnonzero(head)
    ep = np.concatenate([hp[1:], [len(fo)]])
    sn = np.cumsum(head) - 1
    pos = np.zeros(len(fo), dtype=STREAM_POS_DTYPE)
    pos["stream"][order] = sn
    pos["pos"][order] = (np.arange(len(fo)) - hp[sn]) * L
    recs = np.zeros(len(hp), dtype=STREAM_DTYPE)
    recs["first_packet"], recs["last_packet"], recs["n_packets"] = order[hp], order[ep - 1], ep - hp
    recs["bytes"] = (ep - hp) * L
    recs["flow"], recs["dir"] = ks[hp] >> np.uint64(1), ks[hp] & np.uint64(1)
    recs["len"] = np.minimum(recs["bytes"], depth)
    return recs, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--depth", type=int, default=1 << 30)
    ap.add_argument("--scan-depth", type=int, default=1 << 20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams.txt"))
    args = ap.parse_args()
    n, L, stride, depth = args.payloads, 1500, 1504, args.depth
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"flow streams (kmpgpu_load_streams), {n} x {L} B, depth {depth}, medians of {args.reps} rounds with min / quartiles / max, ms "
             f"(GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    ms = {"b": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    st, sel = GpuMatcher(0), GpuMatcher(0)
    seams = {key: (matcher_on(args.parent_lib) if key == "a" else GpuMatcher(0)) for key in ms}
    everyone = list(ms.values()) + [st, sel] + list(seams.values())
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
        for m in [st] + list(seams.values()):
            m.set_patterns(tokens)
        st.set_rules(rules)

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

        by_turns(f"(1) kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules, (a) parent (b) this tree",
                 {key: (lambda m=m: m.scan_rules(hits=True)) for key, m in ms.items()}, same_rules)
        ones = np.full((n + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        d_ones = torch.from_numpy(ones.view(np.int64)).cuda()
        for shape in ("one flow", "10 000 flows, Zipf sizes", "every payload its own flow"):
            flow = gen_flows(shape, n)
            meta = gen_meta(flow)
            d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1).copy()).cuda()
            for m in ms.values():
                m.set_meta(d_meta)
                assert m.build_flows() == int(flow.max()) + 1
            # ---- (1) an unchanged loader
            def same_seams(res):
                if "a" in res:
                    assert res["a"] == res["b"] and seams["a"].seams().tobytes() == seams["b"].seams().tobytes()
            by_turns(f"(1) {shape}, kmpgpu_load_seams(reach 98), (a) parent (b) this tree",
                     {key: (lambda key=key: seams[key].load_seams(ms[key], 98)) for key in ms}, same_seams)
            # ---- (2) the build, kernel by kernel, with the selection's copy and the seams in the same rounds
            want, want_pos = host_streams(meta, b.flow_ids(), b.flows()["first"], depth, L)
            n_streams = st.load_streams(b, depth)
            assert n_streams == len(want) and st.streams().tobytes() == want.tobytes() and st.stream_map().tobytes() == want_pos.tobytes(), \
                "kmpgpu_load_streams and numpy disagree"
            tt, kk, ss, mm = [], [], [], []
            for rnd in range(3 + args.reps):
                st.profile_begin(16)
                st.load_streams(b, depth)
                prof = st.profile_end(16)
                # (the C call: the Python wrapper would copy a device bitmap to the host to return the indices)
                _lib.gpu_check(sel._g.kmpgpu_load_selected(sel._ctx, b._ctx, d_ones.data_ptr(), 1, None), "kmpgpu_load_selected")
                seams["b"].load_seams(b, 98)
                if rnd >= 3:
                    tt.append(st.last_timing().kernel_ms); kk.append(prof)
                    ss.append(sel.last_timing().kernel_ms); mm.append(seams["b"].last_timing().kernel_ms)
            names = ("keys", "sort", "stream scan + totals", "heads + records + slot scan x 2", "index", "gather")
            per = ", ".join(f"{nm} {statistics.median([k[i] for k in kk]):.3f}" for i, nm in enumerate(names) if all(len(k) > i for k in kk))
            g, s_med = statistics.median([k[5] for k in kk]), statistics.median(ss)
            nbytes, sel_bytes = st.arena_info()[1], sel.arena_info()[1]
            say(f"(2) {shape} ({n_streams} streams, {nbytes} bytes; kernel_ms of kmpgpu_last_timing): kmpgpu_load_streams {spread(tt)}; kernels: {per}; "
                f"the gather moves 2 x {nbytes} bytes at {2 * nbytes / g / 1e6:.0f} GB/s; kmpgpu_load_selected, all bits ({sel_bytes} bytes): "
                f"{spread(ss)}; gather / load_selected {g / s_med:.2f}, load_streams / load_selected {statistics.median(tt) / s_med:.2f}; "
                f"kmpgpu_load_seams(reach 98): {spread(mm)}")
            # ---- (3) the flow verdict on the streams against the seams' route
            st.load_streams(b, args.scan_depth)
            assert st.build_flows() == int(flow.max()) + 1 and st.flow_ids().tolist() == want["flow"].tolist()
            by_turns(f"(3) {shape}, depth {args.scan_depth} ({st.arena_info()[1]} bytes), (streams) kmpgpu_scan_flows(rules, scope flow) on the stream context, (seams) kmpgpu_scan_flows_seams on src, "
                     f"(b) kmpgpu_scan_flows on src",
                     {"streams": lambda: st.scan_flows("rules", "flow"), "seams": lambda: b.scan_flow_seams(seams["b"]),
                      "b": lambda: b.scan_flows("rules", "flow")})
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
