"""What the chains (kmpgpu_set_chains) cost, and what they save (profiles/chains.txt).

    python3 tools/chains.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/chains.txt]
                            [--bench-parent <file>] [--bench-this <file>]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the contexts alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.
  (1) unchanged path   kmpgpu_scan_rules, strings.txt's 97 tokens and 100 generated rules: (a) the parent commit's library
                       (--parent-lib; left out without it) against (b) this tree's with no chains set.  The outputs must be equal.
  (2) chains           the same rules, 50 chains of three contents over the tokens added, the first 50 rules each with one of them as a
                       further term: (c) kmpgpu_scan_rules of this tree, beside its chain kernel alone (kmpgpu_profile_begin: the launch in
                       front of the rules kernel), against (d) the route there was before: kmpgpu_scan_offsets, the records downloaded,
                       and the join on the host with numpy, link by link (sorted keys payload << 32 | offset of the starts reached so
                       far, two binary searches per record of the next content).  (d) gives the chain rows only, not yet the rules over
                       them.  The rows must be equal.  (d) takes thousands of times as long as (c), so it is run in every tenth round
                       only (the output names the number of calls), its min / quartiles / max are of those.
  (3) dense            text over {a, b} and the two patterns "ab" and "ba": every payload is a candidate of every chain.
                       kmpgpu_scan_chains and its chain kernel alone, per chain and payload.
--bench-parent / --bench-this: files that hold the JSON line `python bench.py` printed on the parent commit and on this tree in the
same session; they are copied into the output."""
import argparse
import ctypes as C
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
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402


def matcher_on(path):
    """a GpuMatcher on another build of the library (one without kmpgpu_set_chains included)"""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.GPU_API.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    return GpuMatcher(0, lib=lib)


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def spread(v):
    q = statistics.quantiles(v, n=4)
    return f"{statistics.median(v):.3f} (min {min(v):.3f} q1 {q[0]:.3f} q3 {q[2]:.3f} max {max(v):.3f})"


def gen_rules(rng, n_rules, n_pat):
    """as tools/rules.py"""
    rules = []
    for _ in range(n_rules):
        pos, neg = [], []
        for _ in range(rng.randrange(1, 5)):
            (neg if rng.random() < 0.25 else pos).append(rng.randrange(n_pat))
        rules.append((pos, neg))
    return rules


def gen_chains(rng, n_chains, pkt_counts):
    """three patterns that hit somewhere, with the bounds a signature carries: within a few dozen bytes behind, anywhere behind, in front"""
    live = [i for i, c in enumerate(pkt_counts) if c]
    chains = []
    for q in range(n_chains):
        a, b, c = rng.choice(live), rng.choice(live), rng.choice(live)
        w = rng.randrange(8, 200)
        chains.append([(a, (b, 0, w), (c, 0, w)), (a, (b, 0, None), (c, 0, w)), (a, (b, None, -1), (c, 0, None)), (a, (b, -64, 64), (c, -64, 64))][q % 4])
    return chains


def host_join(recs, pat_len, chains, n_pkts):
    """the chain rows from the records of kmpgpu_scan_offsets: bool[n_chains, n_pkts]"""
    pat = recs["pattern"]
    order = np.argsort(pat, kind="stable")
    bounds = np.searchsorted(pat[order], np.arange(len(pat_len) + 1))
    cache = {}

    def of(i):
        if i not in cache:
            r = recs[order[bounds[i]:bounds[i + 1]]]
            cache[i] = (r["packet"].astype(np.int64), r["offset"].astype(np.int64))
        return cache[i]

    rows = np.zeros((len(chains), n_pkts), dtype=bool)
    for q, ch in enumerate(chains):
        prev = ch[0]
        pk, so = of(prev)
        for p, lo, hi in ch[1:]:
            keys = np.sort((pk << 32) | so)                      # the starts of the content before that a tuple reaches
            pb, sb = of(p)
            if not len(keys) or not len(pb):
                pk = pb[:0]
                break
            first = np.maximum(sb - pat_len[prev] - (hi if hi is not None else 1 << 31), 0)
            last = sb - pat_len[prev] - (lo if lo is not None else -(1 << 31))
            ok = last >= first
            last = np.minimum(last, (1 << 32) - 1)
            n_in = np.searchsorted(keys, (pb << 32) | last, side="right") - np.searchsorted(keys, (pb << 32) | first, side="left")
            keep = ok & (n_in > 0)
            pk, so, prev = pb[keep], sb[keep], p
        rows[q, pk] = True
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-this", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chains.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"chains (kmpgpu_set_chains), {n} x {L} B, medians of {args.reps} alternating rounds with min / quartiles / max, ms "
             f"(GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    ms = {"b": GpuMatcher(0), "c": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    try:
        for m in ms.values():
            m.set_stream(stream.cuda_stream)
        b, c = ms["b"], ms["c"]
        b.fixed_index(d_off, d_len, L, 16)
        b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=needle, plant_permille=100))
        b.sync()
        n_pat = len(tokens)
        rules = gen_rules(random.Random(100), 100, n_pat)
        for m in ms.values():
            m.set_patterns(tokens)
            m.attach_arena(d_arena, d_off, d_len)
        pk = b.scan_packets()
        chains = gen_chains(random.Random(50), 50, pk["pkt_counts"].tolist())
        c.set_chains(chains)
        rules_c = [(pos + [c.chain(r)], neg) if r < len(chains) else (pos, neg) for r, (pos, neg) in enumerate(rules)]
        for key, m in ms.items():
            m.set_rules(rules_c if key == "c" else rules)
        # ---- (1) the unchanged path
        res = {key: m.scan_rules(hits=True) for key, m in ms.items() if key != "c"}
        if "a" in res:
            for k in ("hits", "rule_pkt_counts", "any", "counts"):
                assert np.array_equal(res["a"][k], res["b"][k]), k
        # ---- (2): what the chains are, and the host's rows against the device's
        rel = c.scan_chains(hits=True)
        c.set_chains([(ch[0],) + tuple((p, None, None) for p, _, _ in ch[1:]) for ch in chains])
        cand = c.scan_chains()["chain_pkt_counts"]
        c.set_chains(chains)
        c.set_rules(rules_c)
        total = int(rel["counts"].sum())
        pat_len = [len(t) for t in tokens]

        def host_route():
            t0 = time.perf_counter()
            recs, found, _ = c.scan_offsets(total)
            t1 = time.perf_counter()
            rows = host_join(recs, pat_len, chains, n)
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, rows, found

        _, _, rows, found = host_route()
        assert found == total and np.array_equal(rows, rel["hits"]), "the host join and the chain kernel disagree"

        def rules_profiled(m):
            m.profile_begin(64)
            dt, r = timed(stream, lambda: m.scan_rules())
            return dt, r["timing"].kernel_ms, m.profile_end(64)

        t = {key: [] for key in ms}
        own = {key: [] for key in ms}
        relk, rulk, off_ms, join_ms = [], [], [], []
        for rnd in range(3 + args.reps):                                 # three rounds of warm-up
            for key, m in ms.items():
                if key == "c":
                    dt, k_ms, prof = rules_profiled(m)
                    if rnd >= 3:
                        relk.append(prof[-2]); rulk.append(prof[-1])
                else:
                    dt, r = timed(stream, lambda: m.scan_rules())
                    k_ms = r["timing"].kernel_ms
                if rnd >= 3:
                    t[key].append(dt); own[key].append(k_ms)
            if rnd >= 3 and rnd % 10 == 3:                               # the host route takes thousands of times as long: every tenth round
                o, j, _, _ = host_route()
                off_ms.append(o); join_ms.append(j)
        line = f"(1) kmpgpu_scan_rules, {n_pat} tokens, {len(rules)} rules, no chains set: "
        if "a" in t:
            line += f"(a) parent {spread(t['a'])}, kernel_ms {statistics.median(own['a']):.3f}; "
        line += f"(b) this tree {spread(t['b'])}, kernel_ms {statistics.median(own['b']):.3f}"
        if "a" in t:
            mb = statistics.median(t["b"])
            line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
        say(line)
        say(f"(2) the same with {len(chains)} chains of three contents, one more term in each of the first {len(chains)} rules: {int(cand.sum())} candidates "
            f"(payload, chain) -- {int(cand.sum()) / len(chains) / n * 100:.2f} % of the payloads per chain --, {int(rel['chain_pkt_counts'].sum())} of them hold; "
            f"(c) kmpgpu_scan_rules {spread(t['c'])}, kernel_ms {statistics.median(own['c']):.3f}; (c) - (b) {statistics.median(t['c']) - statistics.median(t['b']):.3f}; "
            f"chain kernel alone {spread(relk)}, rules kernel alone {statistics.median(rulk):.3f}")
        say(f"    (d) the host route, {len(off_ms)} calls: kmpgpu_scan_offsets with its download of {total} records {spread(off_ms)}, the numpy join "
            f"{spread(join_ms)}; (d) / (c) {(statistics.median(off_ms) + statistics.median(join_ms)) / statistics.median(t['c']):.1f}")
        # ---- (3) dense
        c.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=99, needle=b"a", plant_permille=0, lo=ord("a"), span=2))
        c.sync()
        dense = [(0, (1, 0, 10), (0, 0, 10)), (1, (0, None, None), (1, None, None)), (0, (0, 600, 650), (0, 600, 650)), (0, (1, -700, -690), (0, 1390, 1400))]
        c.set_patterns([b"ab", b"ba"])
        c.attach_arena(d_arena, d_off, d_len)
        c.set_chains(dense)
        res = c.scan_chains()
        c.set_chains([(ch[0],) + tuple((p, None, None) for p, _, _ in ch[1:]) for ch in dense])
        cand = c.scan_chains()["chain_pkt_counts"]
        c.set_chains(dense)
        td, kd, pkd = [], [], []
        for rnd in range(3 + args.reps):
            c.profile_begin(64)
            dt, _ = timed(stream, lambda: c.scan_chains())
            prof = c.profile_end(64)
            dp, _ = timed(stream, lambda: c.scan_packets())
            if rnd >= 3:
                td.append(dt); kd.append(prof[-1]); pkd.append(dp)
        per = statistics.median(kd) * 1e6 / max(int(cand.sum()), 1)
        say(f"(3) dense: text over {{a, b}}, patterns 'ab' and 'ba', {len(dense)} chains {dense}: {int(cand.sum())} candidates "
            f"({int(cand.sum()) / len(dense) / n * 100:.1f} % of the payloads per chain), {int(res['chain_pkt_counts'].sum())} hold; kmpgpu_scan_chains "
            f"{spread(td)}; chain kernel alone {spread(kd)} = {per:.1f} ns per candidate, {n * L * len(dense) / statistics.median(kd) / 1e6:.0f} GB/s of "
            f"candidate payload bytes; kmpgpu_scan_packets on the same arena {statistics.median(pkd):.3f}")
    finally:
        for m in ms.values():
            m.close()
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    for name, path in (("parent commit", args.bench_parent), ("this tree", args.bench_this)):
        if path:
            with open(path) as f:
                out = [x for x in f.read().splitlines() if x.startswith("{")]
            say(f"python bench.py, {name}: {out[-1] if out else 'no result line'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
