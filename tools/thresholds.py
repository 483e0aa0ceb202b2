"""What rate thresholds cost (profiles/thresholds.txt).

    python3 tools/thresholds.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 10] [--out profiles/thresholds.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, strings.txt's 97 tokens and 100 generated
rules, HIP events on the contexts' stream around each call, the contexts alternating inside every round so that drift hits them alike;
medians of --reps rounds after a warm-up, with the smallest, the quartiles and the largest.  The metadata is that of tools/flows.py;
timestamps in microseconds with random gaps of 1 ms on average, windows of 60 ms.  Three setups: ONE tracker (by_rule), 10 000 trackers
with Zipf sizes (by_flow and by_src), every payload its own tracker (by_flow and by_src).
  (1) unchanged paths  kmpgpu_scan_rules and kmpgpu_scan_flowbits: the parent commit's library (--parent-lib; left out without it)
                       against this tree's, in the same rounds, before and after the threshold calls.  The outputs must be equal, and
                       this tree's median has to lie inside the parent's own run-to-run range, which the line states.
  (2) scan_thresholds  per setup the whole call -- timestamps already on the device, no rows downloaded: what the kernels cost -- and its own kernels from kmpgpu_profile_begin: the max-scan of the timestamps, per sorted
                       track the order (keys, sort and heads; only in the first call) and T in its order, per threshold the count (gather
                       and prefix sum) and the pass kernel, then the final pass.  What lies in front of them in the profile is the pass
                       of kmpgpu_scan_rules.  The alert rows are checked against (3).
  (3) today's route    like for like, wall clock, medians of 5 runs: timestamps on the host in, alert rows as a bool matrix on the host
                       out.  The call: scan_thresholds(ts, hits=True).  Today: scan_rules(hits=True), then per threshold a stable argsort
                       by tracker, a cumsum and one searchsorted over (tracker, T) with numpy; the trackers' keys of the tracks in use are
                       made outside the clock.  Both routes download and unpack the same number of rows."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

from flows import gen_flows, gen_meta  # noqa: E402  (tools/flows.py: the same shapes)
from headers import gen_rules, matcher_on, spread, timed  # noqa: E402  (tools/headers.py: the same instrument)

WINDOW = 60_000               # microseconds
TRACKS = ("by_rule", "by_src", "by_dst", "by_flow")
FLOWBITS = [(0, "isnotset", 0), (0, "set", 0)]
HOST_REPS = 5


def host_thresholds(base, ts, thr, keys):
    """alert rows bool[n_rules, n]: times below 2^40 and trackers below 2^23, so (tracker, T) is one 64-bit key"""
    n = base.shape[1]
    T = np.maximum.accumulate(ts)
    assert int(T[-1]) < 1 << 40
    alert = base.copy()
    for rule, track, kind, count, window in thr:
        key = keys[track].astype(np.uint64)
        assert int(key.max()) < 1 << 23
        order = np.argsort(key, kind="stable")
        both = key[order] << np.uint64(40) | T[order]
        C = np.concatenate(([0], np.cumsum(base[rule][order])))
        edge = key[order] << np.uint64(40) | np.where(T[order] >= np.uint64(window), T[order] - np.uint64(window), np.uint64(0))
        lo = np.where(T[order] >= np.uint64(window), np.searchsorted(both, edge, side="right"), np.searchsorted(both, edge, side="left"))
        cnt = C[np.arange(n) + 1] - C[lo]
        ok = cnt >= count if kind == "at_least" else cnt <= count if kind == "at_most" else cnt == count
        back = np.zeros(n, dtype=bool)
        back[order] = ok
        alert[rule] &= back
    return alert


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thresholds.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"rate thresholds (kmpgpu_set_thresholds, kmpgpu_scan_thresholds), {n} x {L} B, medians of {args.reps} rounds with min / quartiles / max, "
             f"ms (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    ms = {"b": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    try:
        for m in ms.values():
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
        ts = np.cumsum(np.random.default_rng(7).integers(0, 2001, n)).astype(np.uint64)
        d_ts = torch.from_numpy(ts.view(np.int64)).cuda()

        def by_turns(label, calls, equal):
            """calls: {key: function}; equal(a, b) checks the results of "a" and "b" """
            res = {key: fn() for key, fn in calls.items()}
            if "a" in res and "b" in res:
                equal(res["a"], res["b"])
            t = {key: [] for key in calls}
            for rnd in range(3 + args.reps):
                for key, fn in calls.items():
                    dt, _ = timed(stream, fn)
                    if rnd >= 3:
                        t[key].append(dt)
            line = f"{label}: " + "; ".join(f"({key}) {spread(v)}" for key, v in t.items())
            if "a" in t and "b" in t:
                mb = statistics.median(t["b"])
                line += (f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; the parent's range {min(t['a']):.3f} .. {max(t['a']):.3f}, "
                         f"(b)'s median inside it: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}")
            say(line)

        def same(keys):
            def check(x, y):
                for k in keys:
                    assert np.array_equal(x[k], y[k]), k
                assert x["timing"].launches == y["timing"].launches
            return check

        def unchanged(when):
            for m in ms.values():
                m.scan_flowbits()                          # (whoever calls first after a build of the flows sorts them: not part of the comparison)
            by_turns(f"(1) {when}: kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules, (a) parent (b) this tree",
                     {key: (lambda m=m: m.scan_rules(hits=True)) for key, m in ms.items()}, same(("hits", "any", "counts", "rule_pkt_counts")))
            by_turns(f"(1) {when}: kmpgpu_scan_flowbits, fire once on rule 0, (a) parent (b) this tree",
                     {key: (lambda m=m: m.scan_flowbits(hits=True)) for key, m in ms.items()},
                     same(("hits", "any", "counts", "rule_pkt_counts", "flow_state")))

        setups = [("one tracker", "one flow", [(0, "by_rule", "at_least", 5, WINDOW), (1, "by_rule", "at_most", 1, WINDOW)]),
                  ("10 000 trackers, Zipf sizes", "10 000 flows, Zipf sizes", [(0, "by_flow", "at_least", 5, WINDOW), (1, "by_src", "at_most", 1, WINDOW)]),
                  ("1 M trackers", "every payload its own flow", [(0, "by_flow", "at_least", 1, WINDOW), (1, "by_src", "at_most", 1, WINDOW)])]
        for i, (name, shape, thr) in enumerate(setups):
            flow = gen_flows(shape, n)
            meta = gen_meta(flow)
            d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1).copy()).cuda()
            for m in ms.values():
                m.set_meta(d_meta)
                assert m.build_flows() == int(flow.max()) + 1
                m.set_flowbits(FLOWBITS)
            if i == 0:
                unchanged("before any threshold call")
            sorted_tracks = len({t[1] for t in thr} - {"by_rule"})
            own = 1 + sorted_tracks + 2 * len(thr) + 1
            b.set_thresholds(thr)
            b.build_flows()                                # a new generation: the next call sorts the flows
            b.profile_begin(64)
            res = b.scan_thresholds(d_ts, hits=True)
            first = b.profile_end(64)
            tt, kk = [], []
            for rnd in range(3 + args.reps):
                b.profile_begin(64)
                dt, _ = timed(stream, lambda: b.scan_thresholds(d_ts, hits=False))          # timestamps on the device, no rows downloaded
                prof = b.profile_end(64)
                if rnd >= 3:
                    tt.append(dt); kk.append(prof[-own:])
            med = [statistics.median([k[j] for k in kk]) for j in range(own)]
            # the thresholds are launched track by track: by_rule, by_src, by_dst, by_flow
            launched = sorted(range(len(thr)), key=lambda q: (TRACKS.index(thr[q][1]), q))
            per = "; ".join(f"threshold {q} ({thr[q][1]}): count {med[1 + sorted_tracks + 2 * j]:.3f} pass {med[2 + sorted_tracks + 2 * j]:.3f}"
                            for j, q in enumerate(launched))
            say(f"(2) {name}: kmpgpu_scan_thresholds, timestamps on the device and the rows left there, {spread(tt)}, {res['timing'].launches} launches in the first call ({len(first)} profiled), "
                f"{len(prof)} profiled later; max-scan of ts {med[0]:.3f}; T into "
                f"{sorted_tracks} sorted orders {sum(med[1:1 + sorted_tracks]):.3f}; {per}; final pass {med[-1]:.3f}; its kernels together {sum(med):.3f}")
            if sorted_tracks:
                # in the first call every sorted track has one more entry, its order, in front of its T
                extra = first[len(first) - own - sorted_tracks:]
                orders = [extra[1 + 2 * s] for s in range(sorted_tracks)]
                say(f"    {name}: the orders, first call only (keys, sort, heads): " + ", ".join(f"{v:.3f}" for v in orders))
            # like for like: both routes start from timestamps on the host and end with the alert rows as a bool matrix on the host.
            # The trackers' keys of the setup's tracks are made outside the clock (the caller of either route has them or needs none)
            keys = {}
            for track in {t[1] for t in thr}:
                keys[track] = (np.zeros(n, dtype=np.int64) if track == "by_rule" else b.flow_ids().astype(np.int64) if track == "by_flow"
                               else np.unique(meta["src_ip" if track == "by_src" else "dst_ip"], return_inverse=True)[1])
            gpu_wall, host_wall = [], []
            for rnd in range(1 + HOST_REPS):
                t0 = time.perf_counter()
                got = b.scan_thresholds(ts, hits=True)["hits"]
                t1 = time.perf_counter()
                rows = b.scan_rules(hits=True)["hits"]
                t2 = time.perf_counter()
                want = host_thresholds(rows, ts, thr, keys)
                t3 = time.perf_counter()
                assert np.array_equal(want, got) and np.array_equal(got, res["hits"]), "kmpgpu_scan_thresholds and the host route disagree"
                if rnd:
                    gpu_wall.append((t1 - t0) * 1e3); host_wall.append(((t2 - t1) * 1e3, (t3 - t2) * 1e3))
            g, hr, hn = statistics.median(gpu_wall), statistics.median(h[0] for h in host_wall), statistics.median(h[1] for h in host_wall)
            say(f"(3) {name}, wall clock, medians of {HOST_REPS} runs, timestamps from the host, alert rows to the host as a bool matrix: "
                f"scan_thresholds(ts, hits=True) {g:.1f} ms; today's route {hr + hn:.1f} ms = scan_rules(hits=True) {hr:.1f} + argsort, cumsum and "
                f"searchsorted with numpy {hn:.1f}; the same alert rows; today's route / the call {(hr + hn) / g:.2f}")
            b.set_thresholds([])
        unchanged("after the threshold calls")
    finally:
        for m in ms.values():
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
