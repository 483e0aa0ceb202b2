"""What the byte tests (kmpgpu_set_bytetests) cost (profiles/bytetests.txt).

    python3 tools/bytetests.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/bytetests.txt]
                               [--bench-parent <file>] [--bench-this <file>]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the contexts alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.
  (1) unchanged path    kmpgpu_scan_rules, strings.txt's 97 tokens and 100 generated rules: (a) the parent commit's library
                        (--parent-lib; left out without it) against (b) this tree's with no byte tests set.  The outputs must be
                        equal.  What is claimed is "within the run-to-run spread of the parent": both spreads are printed.
  (2) absolute kernel   1, 100 and 1 000 absolute tests at offsets below 64, under the strlen rule and under whole payloads:
                        kmpgpu_scan_bytetests, and the kernel alone from kmpgpu_profile_begin (the last launch), beside the bytes it must
                        move -- 12 bytes of index per payload, n_bt x W2 x 8 written; the field dwords and the first 64 bytes of text are
                        extra -- .  The rows of the first 4 096 payloads are checked against a Python evaluation of the definition.
  (3) relative kernel   16 tests behind one anchor (the bench needle) that lies in every tenth payload, then in every payload: the
                        kernel alone (the last launch), per candidate payload.
--bench-parent / --bench-this: files that hold the JSON lines `python bench.py` printed on the parent commit and on this tree, run by
turns in one session; every run's rate and step time are copied into the output, the last line of each in full."""
import argparse
import ctypes as C
import json
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
from multithreading_string_matching_amd.host import BYTETEST_DTYPE  # noqa: E402
from multithreading_string_matching_amd.matcher import OPT_WHOLE_PAYLOAD, GpuMatcher  # noqa: E402

HBM_PEAK = 8.0e12                 # bytes / s, data sheet (what the other profiles' fractions are of)
CHECKED = 4096                    # payloads whose rows are held to the definition


def matcher_on(path):
    """a GpuMatcher on another build of the library (one without kmpgpu_set_bytetests included)"""
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


def gen_tests(n_bt, relative, seed=9):
    """tests over text of a..z: fields compared with values made of letters, so that a row holds a share of the payloads"""
    rng = np.random.default_rng(seed)
    t = np.zeros(n_bt, dtype=BYTETEST_DTYPE)
    t["nbytes"] = rng.integers(1, 5, n_bt)
    t["op"] = rng.integers(0, 6, n_bt)
    t["flags"] = rng.integers(0, 2, n_bt) * _lib.BT_LITTLE | (_lib.BT_RELATIVE if relative else 0)
    t["offset"] = rng.integers(-8, 24, n_bt) if relative else rng.integers(0, 61, n_bt)
    t["mask"] = rng.choice([0xFFFFFFFF, 0xFFFFFFFF, 0x1F1F1F1F], n_bt)
    letters = rng.integers(0x61, 0x7B, (n_bt, 4)).astype(np.uint32)
    value = (letters[:, 0] << 24 | letters[:, 1] << 16 | letters[:, 2] << 8 | letters[:, 3]) >> (8 * (4 - t["nbytes"].astype(np.uint32)))
    t["value"] = value & t["mask"]
    return t


def row_of(payloads, t, starts, m):
    """test t over the payloads (uint8[n, L], no 0x00 in them), from the definition in include/kmpgpu.h; starts[k]: where the anchor starts"""
    n, L = payloads.shape
    out = np.zeros(n, dtype=bool)
    little = bool(int(t["flags"]) & _lib.BT_LITTLE)
    nb, mask, value, op = int(t["nbytes"]), int(t["mask"]), int(t["value"]), int(t["op"])
    for k in range(n):
        for s in (starts[k] if int(t["flags"]) & _lib.BT_RELATIVE else [-m]):
            pos = s + m + int(t["offset"])
            if pos < 0 or pos + nb > L:
                continue
            f = int.from_bytes(payloads[k, pos:pos + nb].tobytes(), "little" if little else "big") & mask
            if [f == value, f != value, f < value, f > value, f <= value, f >= value][op]:
                out[k] = True
                break
    return out


def raw_rows(m, n_bt, n):
    """(bt_pkt_counts, rows as uint64[n_bt, W]) of kmpgpu_scan_bytetests: the words as they come"""
    W = (n + 63) // 64
    pc, hit_w = np.zeros(n_bt, dtype=np.uint64), np.zeros((n_bt, W), dtype=np.uint64)
    _lib.gpu_check(m._g.kmpgpu_scan_bytetests(m._ctx, pc.ctypes.data, None, hit_w.ctypes.data, None, None), "kmpgpu_scan_bytetests")
    return pc, hit_w


def check_rows(m, tests, head, starts, needle_len, n):
    pc, hit_w = raw_rows(m, len(tests), n)
    for q in sorted({0, len(tests) // 2, len(tests) - 1}):
        want = row_of(head, tests[q], starts, needle_len)
        got = np.unpackbits(hit_w[q, :CHECKED // 64].view(np.uint8), bitorder="little").astype(bool)
        assert np.array_equal(got, want), "the byte-test kernel and the definition disagree"
    return float(pc.sum()) / len(tests) / n


def kernel_alone(c, stream, reps):
    tt, kk = [], []
    for rnd in range(3 + reps):
        c.profile_begin(64)
        dt, _ = timed(stream, lambda: c.scan_bytetests())
        prof = c.profile_end(64)
        if rnd >= 3:
            tt.append(dt); kk.append(float(prof[-1]))
    return tt, kk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-this", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bytetests.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    assert n >= CHECKED
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"byte tests (kmpgpu_set_bytetests), {n} x {L} B, medians of {args.reps} alternating rounds with min / quartiles / max, ms "
             f"(GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def head_of_arena():
        """(the first CHECKED payloads as uint8[CHECKED, L], where the needle starts in each)"""
        head = d_arena[:CHECKED * stride].cpu().numpy().reshape(CHECKED, stride)[:, :L]
        starts = []
        for k in range(CHECKED):
            row, s, ss = head[k].tobytes(), 0, []
            while (s := row.find(needle, s)) >= 0:
                ss.append(s)
                s += 1
            starts.append(ss)
        return head, starts

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
        for key, m in ms.items():
            m.set_patterns([needle] if key == "c" else tokens)
            m.attach_arena(d_arena, d_off, d_len)
        # ---- (1) the unchanged path
        for key in ("a", "b"):
            if key in ms:
                ms[key].set_rules(rules)
        res = {key: ms[key].scan_rules(hits=True) for key in ("a", "b") if key in ms}
        if "a" in res:
            for k in ("hits", "rule_pkt_counts", "any", "counts"):
                assert np.array_equal(res["a"][k], res["b"][k]), k
            assert res["a"]["timing"].launches == res["b"]["timing"].launches
        t = {key: [] for key in res}
        own = {key: [] for key in res}
        for rnd in range(3 + args.reps):                                 # three rounds of warm-up
            for key in res:
                dt, r = timed(stream, lambda: ms[key].scan_rules())
                if rnd >= 3:
                    t[key].append(dt); own[key].append(r["timing"].kernel_ms)
        line = f"(1) kmpgpu_scan_rules, {n_pat} tokens, {len(rules)} rules, no byte tests set: "
        if "a" in t:
            line += f"(a) parent {spread(t['a'])}, kernel_ms {statistics.median(own['a']):.3f}; "
        line += f"(b) this tree {spread(t['b'])}, kernel_ms {statistics.median(own['b']):.3f}"
        if "a" in t:
            mb = statistics.median(t["b"])
            line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
        say(line)
        del res
        # ---- (2) the absolute kernel
        head, starts = head_of_arena()
        W2 = ((n + 63) // 64 + 1) & ~1
        for whole in (0, 1):
            c.set_option(OPT_WHOLE_PAYLOAD, whole)
            for n_bt in (1, 100, 1000):
                tests = gen_tests(n_bt, relative=False)
                c.set_bytetests(tests)
                share = check_rows(c, tests, head, starts, len(needle), n)
                tt, kk = kernel_alone(c, stream, args.reps)
                moved = 12 * n + n_bt * W2 * 8
                k_med = statistics.median(kk)
                say(f"(2) {'whole payloads' if whole else 'strlen rule'}, {n_bt} absolute tests ({share * 100:.1f} % of the payloads per test): "
                    f"kmpgpu_scan_bytetests {spread(tt)}; absolute kernel alone {spread(kk)}; index and rows: 12 x {n} + {n_bt} x {W2} x 8 = {moved} "
                    f"bytes, {moved / k_med / 1e6:.1f} GB/s, {moved / (k_med * 1e-3) / HBM_PEAK * 100:.2f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM rate; "
                    f"{k_med * 1e6 / n_bt / n * 1e3:.2f} ps per (test, payload)")
        c.set_option(OPT_WHOLE_PAYLOAD, 0)
        # ---- (3) the relative kernel
        tests = gen_tests(16, relative=True)
        for permille in (100, 1000):
            if permille != 100:
                b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=needle, plant_permille=permille))
                b.sync()
                c.attach_arena(d_arena, d_off, d_len)
                head, starts = head_of_arena()
            c.set_bytetests(tests)
            share = check_rows(c, tests, head, starts, len(needle), n)
            cand = int(c.scan_packets()["pkt_counts"][0])
            tt, kk = kernel_alone(c, stream, args.reps)
            k_med = statistics.median(kk)
            say(f"(3) 16 relative tests, the anchor in {cand} of {n} payloads ({share * 100:.1f} % of the payloads per test): kmpgpu_scan_bytetests "
                f"{spread(tt)}; relative kernel alone {spread(kk)}; {k_med * 1e6 / 16 / max(cand, 1):.2f} ns per (test, candidate payload)")
    finally:
        for m in ms.values():
            m.close()
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    for name, path in (("parent commit", args.bench_parent), ("this tree", args.bench_this)):
        if path:
            with open(path) as f:
                out = [x for x in f.read().splitlines() if x.startswith("{")]
            runs = ", ".join(f"{r['value']:.1f} GB/s ({r['ms_per_step']:.4f} ms per step)" for r in map(json.loads, out))
            say(f"python bench.py, {name}, {len(out)} runs in the order they were made: {runs if out else 'no result line'}")
            if out:
                say(f"    the last one in full: {out[-1]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
