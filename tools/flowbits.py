"""What flow bits cost (profiles/flowbits.txt).

    python3 tools/flowbits.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/flowbits.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, strings.txt's 97 tokens and 100 generated
rules, HIP events on the contexts' stream around each call, the contexts alternating inside every round so that drift hits them alike;
medians of --reps rounds after a warm-up, with the smallest, the quartiles and the largest.  The metadata is that of tools/flows.py, for
its three shapes: ONE flow, 10 000 flows with Zipf sizes, every payload its own flow.
  (1) unchanged paths  kmpgpu_scan_rules and kmpgpu_load_seams: the parent commit's library (--parent-lib; left out without it) against
                       this tree's, before and after the flow-bit calls.  The outputs must be equal, and this tree's median has to lie
                       inside the parent's own run-to-run range, which the line states.
  (2) scan_flowbits    per shape and op set -- 1 bit on 1 level (fire once), 32 bits on 4 levels (40 rules with ops) -- the whole call,
                       and its own kernels from kmpgpu_profile_begin: the order (the sort and the heads kernel; only in the first call
                       after a build of the flows), then per level build / scan / rows, then the final pass.  What lies in front of them
                       in the profile is the pass of kmpgpu_scan_rules.  The alert rows are checked against (3).
  (3) today's route    the same verdicts on the host: scan_rules(hits=True) + flow_ids(), then the definition's loop vectorised with numpy
                       ACROSS flows -- step j handles the j-th payload of every flow --, which is as many steps as the longest flow has
                       payloads; left out for ONE flow (a million sequential steps).  Host time, wall clock, one run."""
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

TESTS = {"isset": 1, "isnotset": 0}


def op_sets():
    """name -> (ops, n_bits, levels)"""
    deep = []
    for r in range(8):
        deep += [(r, ("set", "toggle")[r % 2], r),
                 (8 + r, "isset", r), (8 + r, "toggle", 8 + r), (8 + r, "noalert"),
                 (16 + r, "isset", 8 + r), (16 + r, "toggle", 16 + r), (16 + r, "noalert"),
                 (24 + r, "isnotset", 16 + r), (24 + r, "set", 24 + r),
                 (32 + r, "isset", 24 + r)]
    return {"1 bit, 1 level": ([(0, "isnotset", 0), (0, "set", 0)], 1, 1), "32 bits, 4 levels": (deep, 32, 4)}


def host_flowbits(base, fo, ops, n_flows):
    """alert rows bool[n_rules, n]: the definition's loop, one step per position inside a flow, all flows at once"""
    n_rules, n = base.shape
    by_rule, noalert = {}, set()
    for op in ops:
        if op[1] == "noalert":
            noalert.add(op[0])
        else:
            by_rule.setdefault(op[0], []).append((op[1], op[2]))
    order = np.argsort(fo, kind="stable")
    sf = fo[order]
    head = np.ones(n, dtype=bool)
    head[1:] = sf[1:] != sf[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    rank = np.arange(n) - start
    by_rank = np.argsort(rank, kind="stable")
    cuts = np.flatnonzero(np.diff(rank[by_rank], prepend=-1))
    S = np.zeros(n_flows, dtype=np.uint32)
    alert = base.copy()
    for r in range(n_rules):
        if r in by_rule and any(w in TESTS for w, _ in by_rule[r]):
            alert[r] = False
    for j, lo in enumerate(cuts):
        hi = cuts[j + 1] if j + 1 < len(cuts) else n
        idx = order[by_rank[lo:hi]]
        f = fo[idx]
        B = S[f]
        new = B.copy()
        for r in sorted(by_rule):
            fired = base[r, idx]
            if not fired.any():
                continue
            for what, X in by_rule[r]:
                if what in TESTS:
                    fired = fired & (((B >> np.uint32(X)) & np.uint32(1)) == TESTS[what])
            alert[r, idx] = fired
            for what, X in by_rule[r]:
                bit = np.uint32(1 << X)
                if what == "set":
                    new = np.where(fired, new | bit, new)
                elif what == "unset":
                    new = np.where(fired, new & ~bit, new)
                elif what == "toggle":
                    new = np.where(fired, new ^ bit, new)
        S[f] = new
    for r in noalert:
        alert[r] = False
    return alert


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowbits.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"flow bits (kmpgpu_set_flowbits, kmpgpu_scan_flowbits), {n} x {L} B, medians of {args.reps} rounds with min / quartiles / max, ms "
             f"(GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    ms = {"b": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    sms = {key: GpuMatcher(0, lib=m._g) for key, m in ms.items()}          # the seams' contexts, each on its source's build
    try:
        for m in list(ms.values()) + list(sms.values()):
            m.set_stream(stream.cuda_stream)
        b = ms["b"]
        b.fixed_index(d_off, d_len, L, 16)
        b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=b"NEEDLE_16B_PATRN", plant_permille=100))
        b.sync()
        rules = gen_rules(random.Random(100), 100, len(tokens))
        for key, m in ms.items():
            m.set_patterns(tokens)
            m.attach_arena(d_arena, d_off, d_len)
            m.set_rules(rules)
            sms[key].set_patterns(tokens)

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

        def same_rules(x, y):
            for k in ("hits", "any", "counts", "rule_pkt_counts"):
                assert np.array_equal(x[k], y[k]), k
            assert x["timing"].launches == y["timing"].launches

        def unchanged(when):
            by_turns(f"(1) {when}: kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules, (a) parent (b) this tree",
                     {key: (lambda m=m: m.scan_rules(hits=True)) for key, m in ms.items()}, same_rules)

        unchanged("before any flow-bit call")
        for shape in ("one flow", "10 000 flows, Zipf sizes", "every payload its own flow"):
            flow = gen_flows(shape, n)
            d_meta = torch.from_numpy(gen_meta(flow).view(np.uint8).reshape(-1).copy()).cuda()
            for m in ms.values():
                m.set_meta(d_meta)
                assert m.build_flows() == int(flow.max()) + 1
            fo = b.flow_ids()
            assert np.array_equal(fo, flow)

            def load(key):
                return sms[key].load_seams(ms[key], 98), sms[key].last_timing().launches

            def same_seams(x, y):
                assert x == y and sms["a"].seams().tobytes() == sms["b"].seams().tobytes()
            by_turns(f"(1) {shape}: kmpgpu_load_seams, reach 98, (a) parent (b) this tree", {key: (lambda key=key: load(key)) for key in ms}, same_seams)
            base = b.scan_rules(hits=True)["hits"]
            for name, (ops, n_bits, levels) in op_sets().items():
                b.set_flowbits(ops, n_bits)
                own = 1 + 3 * levels
                b.build_flows()                            # a new generation: the next call sorts
                b.profile_begin(64)
                res = b.scan_flowbits(hits=True)
                first = b.profile_end(64)
                tt, kk = [], []
                for rnd in range(3 + args.reps):
                    b.profile_begin(64)
                    dt, _ = timed(stream, b.scan_flowbits)
                    prof = b.profile_end(64)
                    if rnd >= 3:
                        tt.append(dt); kk.append(prof[-own:])
                med = [statistics.median([k[i] for k in kk]) for i in range(own)]
                per = "; ".join(f"level {lv}: build {med[3 * lv]:.3f} scan {med[3 * lv + 1]:.3f} rows {med[3 * lv + 2]:.3f}" for lv in range(levels))
                say(f"(2) {shape}, {name}: kmpgpu_scan_flowbits {spread(tt)}, {res['timing'].launches} launches in the first call; order (sort + heads, "
                    f"first call only) {first[-own - 1]:.3f}; {per}; final pass {med[-1]:.3f}; its kernels together {sum(med):.3f}")
                if shape != "one flow":
                    t0 = time.perf_counter()
                    rows = b.scan_rules(hits=True)["hits"]
                    want = host_flowbits(rows, b.flow_ids().astype(np.int64), ops, int(flow.max()) + 1)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    assert np.array_equal(want, res["hits"]), "kmpgpu_scan_flowbits and the host loop disagree"
                    say(f"(3) {shape}, {name}: scan_rules(hits=True) + flow_ids() + the loop vectorised across flows with numpy: {host_ms:.1f} ms "
                        f"(wall clock, one run), the same alert rows")
                else:
                    assert np.array_equal(res["hits"][40:], base[40:]), "the rows of the rules without ops are kmpgpu_scan_rules'"
            b.set_flowbits([])
        unchanged("after the flow-bit calls")
    finally:
        for m in list(ms.values()) + list(sms.values()):
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
