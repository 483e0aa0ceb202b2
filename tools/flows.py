"""What flows cost (profiles/flows.txt).

    python3 tools/flows.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/flows.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the contexts alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.  The metadata is synthesised here for three shapes: ONE flow (what a per-payload atomic
would pay most for), 10 000 flows with Zipf sizes, every payload its own flow.
  (1) unchanged path   kmpgpu_scan_rules, strings.txt's 97 tokens and 100 generated rules: the parent commit's library (--parent-lib;
                       left out without it) against this tree's before and after flows were built on the context.  The outputs must
                       be equal.
  (2) build            kmpgpu_flows_build per shape, and its kernels one by one from kmpgpu_profile_begin (insert, firsts, the two scan
                       kernels together, number, assign); ids and records are checked against numpy.
  (3) scan_flows       97 tokens + 100 rules in both scopes, per shape, with the fold kernel alone (the entry before the last).
  (4) today's route    the same answers without these calls: meta() downloaded and grouped with numpy on the host, the rules' hit rows
                       downloaded (scan_rules(hits)) and folded through that grouping.  Host time, wall clock."""
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
from multithreading_string_matching_amd.host import META_DTYPE  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

from headers import gen_rules, matcher_on, spread, timed  # noqa: E402  (tools/headers.py: the same instrument)


def gen_flows(shape, n, seed=3):
    """flow number per payload, numbered in the order of first appearance"""
    rng = np.random.default_rng(seed)
    if shape == "one flow":
        return np.zeros(n, dtype=np.int64)
    if shape == "every payload its own flow":
        return np.arange(n, dtype=np.int64)
    p = 1.0 / np.arange(1, 10_001) ** 1.1
    draw = rng.choice(10_000, n, p=p / p.sum())
    _, first, inv = np.unique(draw, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv]


def gen_meta(flow, seed=4):
    """a record per payload: flow f talks from 10.0.0.0 + f, a third of the payloads are answers"""
    rng = np.random.default_rng(seed)
    n = len(flow)
    back = rng.integers(0, 3, n) == 0
    meta = np.zeros(n, dtype=META_DTYPE)
    src, dst, sp, dp = 0x0A000000 + flow, np.full(n, 0xC0A80101), 1024 + flow % 60000, np.full(n, 443)
    meta["src_ip"], meta["dst_ip"] = np.where(back, dst, src), np.where(back, src, dst)
    meta["src_port"], meta["dst_port"] = np.where(back, dp, sp), np.where(back, sp, dp)
    meta["proto"] = 6
    return meta


def host_grouping(meta):
    """today's route: the keys canonicalised and grouped with numpy; ids in the order of first appearance"""
    es = meta["src_ip"].astype(np.uint64) << np.uint64(16) | meta["src_port"].astype(np.uint64)
    ed = meta["dst_ip"].astype(np.uint64) << np.uint64(16) | meta["dst_port"].astype(np.uint64)
    key = np.stack([np.minimum(es, ed), np.maximum(es, ed), meta["proto"].astype(np.uint64)], axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv.reshape(-1)].astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flows.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"flows (kmpgpu_flows_build, kmpgpu_scan_flows), {n} x {L} B, medians of {args.reps} rounds with min / quartiles / max, ms "
             f"(GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

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

        def unchanged(label):
            res = {key: m.scan_rules(hits=True) for key, m in ms.items()}
            if "a" in res:
                for k in ("hits", "rule_pkt_counts", "any", "counts"):
                    assert np.array_equal(res["a"][k], res["b"][k]), k
                assert res["a"]["timing"].launches == res["b"]["timing"].launches
            t = {key: [] for key in ms}
            for rnd in range(3 + args.reps):
                for key, m in ms.items():
                    dt, _ = timed(stream, lambda: m.scan_rules())
                    if rnd >= 3:
                        t[key].append(dt)
            line = f"(1) kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules, {label}: "
            if "a" in t:
                line += f"(a) parent {spread(t['a'])}; "
            line += f"(b) this tree {spread(t['b'])}"
            if "a" in t:
                mb = statistics.median(t["b"])
                line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
            say(line)
            return res["b"]

        packet_rows = unchanged("before any flow call")
        for shape in ("one flow", "10 000 flows, Zipf sizes", "every payload its own flow"):
            flow = gen_flows(shape, n)
            meta = gen_meta(flow)
            b.set_meta(torch.from_numpy(meta.view(np.uint8).reshape(-1).copy()).cuda())
            n_flows = b.build_flows()
            fo = b.flow_ids()
            assert n_flows == int(flow.max()) + 1 and np.array_equal(fo, flow), "kmpgpu_flows_build and the shape disagree"
            recs = b.flows()
            assert np.array_equal(recs["n_packets"], np.bincount(flow)) and np.array_equal(recs["payload_bytes"], np.bincount(flow) * L)
            # ---- (2) the build, kernel by kernel
            tt, kk = [], []
            for rnd in range(3 + args.reps):
                b.profile_begin(16)
                dt, _ = timed(stream, b.build_flows)
                prof = b.profile_end(16)
                if rnd >= 3:
                    tt.append(dt); kk.append(prof)
            names = ("insert", "firsts", "scan x 2", "number", "assign")
            per = ", ".join(f"{nm} {statistics.median([k[i] for k in kk]):.3f}" for i, nm in enumerate(names))
            say(f"(2) {shape} ({n_flows} flows): kmpgpu_flows_build {spread(tt)}; kernels: {per}")
            # ---- (3) the fold in both scopes
            for scope in ("packet", "flow"):
                res = b.scan_flows("rules", scope, hits=True)
                if scope == "packet":
                    want = np.zeros((len(rules), n_flows), dtype=bool)
                    for r in range(len(rules)):
                        want[r, fo[packet_rows["hits"][r]]] = True
                    assert np.array_equal(res["hits"], want), "the fold and numpy disagree"
                tt, ff = [], []
                for rnd in range(3 + args.reps):
                    b.profile_begin(64)
                    dt, _ = timed(stream, lambda: b.scan_flows("rules", scope))
                    prof = b.profile_end(64)
                    if rnd >= 3:
                        tt.append(dt); ff.append(float(prof[-2]))
                say(f"(3) {shape}, kmpgpu_scan_flows(rules, scope {scope}): {spread(tt)}; fold kernel alone {spread(ff)}; "
                    f"{int(res['flow_counts'].sum())} (rule, flow) pairs")
            # ---- (4) the route that exists without these calls
            hh = []
            for _ in range(max(3, args.reps // 10)):
                t0 = time.perf_counter()
                ids = host_grouping(b.meta())
                rows = b.scan_rules(hits=True)["hits"]
                out = np.zeros((len(rules), int(ids.max()) + 1), dtype=bool)
                for r in range(len(rules)):
                    out[r, ids[rows[r]]] = True
                hh.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(ids, fo)
            say(f"(4) {shape}, on the host: meta() + numpy grouping + scan_rules(hits) + fold: median {statistics.median(hh):.1f} ms of {len(hh)} (wall clock)")
        unchanged("after the flow calls, flows built on the context")
    finally:
        for m in ms.values():
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
