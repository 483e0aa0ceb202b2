"""What flow seams cost (profiles/seams.txt).

    python3 tools/seams.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--reach 98] [--out profiles/seams.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the contexts alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.  The metadata is that of tools/flows.py, for its three shapes: ONE flow, 10 000 flows with
Zipf sizes, every payload its own flow (which has no seam).
  (1) unchanged paths  kmpgpu_scan_rules and kmpgpu_scan_flows(rules, scope flow), strings.txt's 97 tokens and 100 generated rules: the
                       parent commit's library (--parent-lib; left out without it) against this tree's.  The outputs must be equal.
  (2) load_seams       kmpgpu_load_seams per shape and its kernels from kmpgpu_profile_begin (keys, sort, pred + the two scan kernels,
                       index, gather); the records are checked against numpy, and the gather's bytes (read + written) per second stand
                       beside a device-to-device copy of as many bytes as the seams' arena (the figure of tools/select.py).
  (3) scan_flows_seams against kmpgpu_scan_flows(rules, scope flow) of this tree and of the parent library, by turns.
  (4) today's route    the same answer built on the host: meta() downloaded and grouped with numpy, the seams' bytes cut out of a
                       download of the arena with numpy, load_arena into the second context, scan_packets(hits) of both and the fold.
                       Host time, wall clock."""
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
from multithreading_string_matching_amd.matcher import SEAM_DTYPE, GpuMatcher  # noqa: E402

from flows import gen_flows, gen_meta, host_grouping  # noqa: E402  (tools/flows.py: the same shapes)
from headers import gen_rules, matcher_on, spread, timed  # noqa: E402  (tools/headers.py: the same instrument)


def host_seams(meta, fo, first_meta, reach, L):
    """the seam records with numpy: a stable sort by (flow, dir) keeps capture order, a payload's predecessor is its neighbour"""
    f1 = first_meta[fo]
    dr = ~((meta["src_ip"] == f1["src_ip"]) & (meta["src_port"] == f1["src_port"]) & (meta["dst_ip"] == f1["dst_ip"])
           & (meta["dst_port"] == f1["dst_port"]))
    key = fo.astype(np.uint64) << np.uint64(1) | dr.astype(np.uint64)
    order = np.argsort(key, kind="stable")
    same = np.zeros(len(fo), dtype=bool)
    same[1:] = key[order[1:]] == key[order[:-1]]
    recs = np.zeros(int(same.sum()), dtype=SEAM_DTYPE)
    nxt = np.sort(order[same])
    pr = np.full(len(fo), -1, dtype=np.int64)
    pr[order[same]] = order[np.flatnonzero(same) - 1]
    recs["prev"], recs["next"] = pr[nxt], nxt
    recs["tail_len"] = recs["head_len"] = min(reach, L)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--reach", type=int, default=98)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seams.txt"))
    args = ap.parse_args()
    n, L, stride, reach = args.payloads, 1500, 1504, args.reach
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"flow seams (kmpgpu_load_seams, kmpgpu_scan_flows_seams), {n} x {L} B, reach {reach}, medians of {args.reps} rounds with min / "
             f"quartiles / max, ms (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    ms = {"b": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    sm = GpuMatcher(0)
    try:
        for m in list(ms.values()) + [sm]:
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
        sm.set_patterns(tokens)

        def by_turns(label, calls, keys=("hits", "any", "counts")):
            """calls: {key: function returning a result dict}; the results of "a" and "b" must be equal"""
            res = {key: fn(True) for key, fn in calls.items()}
            if "a" in res and "b" in res:
                for k in keys:
                    assert np.array_equal(res["a"][k], res["b"][k]), (label, k)
                assert res["a"]["timing"].launches == res["b"]["timing"].launches
            t = {key: [] for key in calls}
            for rnd in range(3 + args.reps):
                for key, fn in calls.items():
                    dt, _ = timed(stream, lambda: fn(False))
                    if rnd >= 3:
                        t[key].append(dt)
            line = f"{label}: " + "; ".join(f"({key}) {spread(v)}" for key, v in t.items())
            if "a" in t and "b" in t:
                mb = statistics.median(t["b"])
                line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
            say(line)
            return t

        by_turns(f"(1) kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules, (a) parent (b) this tree",
                 {key: (lambda hits, m=m: m.scan_rules(hits=hits)) for key, m in ms.items()})
        for shape in ("one flow", "10 000 flows, Zipf sizes", "every payload its own flow"):
            flow = gen_flows(shape, n)
            meta = gen_meta(flow)
            d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1).copy()).cuda()
            for m in ms.values():
                m.set_meta(d_meta)
                assert m.build_flows() == int(flow.max()) + 1
            fo = b.flow_ids()
            by_turns(f"(1) {shape}, kmpgpu_scan_flows(rules, scope flow), (a) parent (b) this tree",
                     {key: (lambda hits, m=m: m.scan_flows("rules", "flow", hits=hits)) for key, m in ms.items()})
            # ---- (2) the build, kernel by kernel
            want = host_seams(meta, fo, b.flows()["first"], reach, L)
            n_seams = sm.load_seams(b, reach)
            assert n_seams == len(want) and sm.seams().tobytes() == want.tobytes(), "kmpgpu_load_seams and numpy disagree"
            tt, kk = [], []
            for rnd in range(3 + args.reps):
                sm.profile_begin(16)
                dt, _ = timed(stream, lambda: sm.load_seams(b, reach))
                prof = sm.profile_end(16)
                if rnd >= 3:
                    tt.append(dt); kk.append(prof)
            names = ("keys", "sort", "pred + scan x 2", "index", "gather")
            per = ", ".join(f"{nm} {statistics.median([k[i] for k in kk]):.3f}" for i, nm in enumerate(names) if all(len(k) > i for k in kk))
            line = f"(2) {shape} ({n_seams} seams): kmpgpu_load_seams {spread(tt)}; kernels: {per}"
            if n_seams:
                nbytes = sm.arena_info()[0] * ((2 * min(reach, L) + 15) // 16 * 16)
                scratch, src_bytes = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), d_arena[:nbytes]
                cc = []
                for rnd in range(3 + args.reps):
                    with torch.cuda.stream(stream):
                        dt, _ = timed(stream, lambda: scratch.copy_(src_bytes, non_blocking=True))
                    if rnd >= 3:
                        cc.append(dt)
                g = statistics.median([k[4] for k in kk])
                line += (f"; the gather moves 2 x {nbytes} bytes at {2 * nbytes / g / 1e6:.0f} GB/s, a device copy of as many at "
                         f"{2 * nbytes / statistics.median(cc) / 1e6:.0f} GB/s ({spread(cc)})")
                del scratch
            say(line)
            # ---- (3) the combined scan against the scan without seams
            calls = {key: (lambda hits, m=m: m.scan_flows("rules", "flow", hits=hits)) for key, m in ms.items()}
            calls["seams"] = lambda hits: b.scan_flow_seams(sm, hits=hits)
            t = by_turns(f"(3) {shape}, (a) parent's / (b) this tree's kmpgpu_scan_flows(rules, scope flow) and (seams) kmpgpu_scan_flows_seams", calls)
            say(f"    (seams) / (b) {statistics.median(t['seams']) / statistics.median(t['b']):.4f}; the seams' own kmpgpu_scan_packets: "
                + (spread([timed(stream, sm.scan_packets)[0] for _ in range(args.reps)]) if n_seams else "no seams"))
            # ---- (4) the route that exists without these calls
            if n_seams:
                hh = []
                for _ in range(max(3, args.reps // 10)):
                    t0 = time.perf_counter()
                    mt = b.meta()
                    ids = host_grouping(mt)
                    recs = host_seams(mt, ids, mt[np.unique(ids, return_index=True)[1]], reach, L)
                    host = d_arena.cpu().numpy()
                    r = min(reach, L)
                    tail = host[:n * stride].reshape(n, stride)[recs["prev"].astype(np.int64), L - r:L]
                    head = host[:n * stride].reshape(n, stride)[recs["next"].astype(np.int64), :r]
                    slot = (2 * r + 15) // 16 * 16
                    arena = np.zeros((len(recs), slot), dtype=np.uint8)
                    arena[:, :r], arena[:, r:2 * r] = tail, head
                    with GpuMatcher(0) as tmp:
                        tmp.set_patterns(tokens)
                        tmp.load_arena(np.concatenate([arena.reshape(-1), np.zeros(64, np.uint8)]), np.arange(len(recs), dtype=np.uint64) * slot,
                                       np.full(len(recs), 2 * r, dtype=np.uint32))
                        seam_rows = tmp.scan_packets(hits=True)["hits"]
                    rows = b.scan_packets(hits=True)["hits"]
                    nf = int(ids.max()) + 1
                    out = np.zeros((len(tokens), nf), dtype=bool)
                    sf = ids[recs["next"].astype(np.int64)]
                    for i in range(len(tokens)):
                        out[i, ids[rows[i]]] = True
                        out[i, sf[seam_rows[i]]] = True
                    hh.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(recs, want)
                say(f"(4) {shape}, on the host: meta() + numpy grouping + seams cut with numpy + load_arena + two scan_packets(hits) + fold: "
                    f"median {statistics.median(hh):.1f} ms of {len(hh)} (wall clock)")
        by_turns("(1) kmpgpu_scan_rules after the seam calls, (a) parent (b) this tree",
                 {key: (lambda hits, m=m: m.scan_rules(hits=hits)) for key, m in ms.items()})
    finally:
        for m in list(ms.values()) + [sm]:
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
