"""What the header predicates (kmpgpu_set_headers) cost (profiles/headers.txt).

    python3 tools/headers.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/headers.txt]
                             [--bench-parent <file>] [--bench-this <file>]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1), contexts on one device arena, HIP events on the contexts' stream around
each call, the contexts alternating inside every round so that drift hits them alike; medians of --reps rounds after a warm-up, with
the smallest, the quartiles and the largest.
  (1) unchanged path   kmpgpu_scan_rules, strings.txt's 97 tokens and 100 generated rules: (a) the parent commit's library
                       (--parent-lib; left out without it) against (b) this tree's with no header predicates set and no metadata.  The
                       outputs must be equal.  What is claimed is "within the run-to-run spread of the parent": both spreads are printed.
  (2) header kernel    metadata drawn from small domains (set on the context with kmpgpu_set_meta from a device tensor), 1, 100 and
                       1 000 predicates drawn from the same domains: kmpgpu_scan_headers, and the header kernel alone from
                       kmpgpu_profile_begin (the last launch), beside the bytes it must move -- 20 bytes read per payload, n_hdr x W2 x 8
                       written -- and the fraction of the 8 TB/s data-sheet HBM rate that these bytes over its time come to.  One
                       predicate's rows are checked against a numpy evaluation of the definition.
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
from multithreading_string_matching_amd.host import HEADER_DTYPE, META_DTYPE  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

HBM_PEAK = 8.0e12                 # bytes / s, data sheet (what the other profiles' fractions are of)
ADDR = [0x0A000001, 0x0A800002, 0xC0A80101, 0xAC100A0A]
PORTS = [0, 53, 80, 1024, 40000, 65535]
MASKS = [0, 0xFFFFFFFF, 0xFF000000, 0xFFFF0000]


def matcher_on(path):
    """a GpuMatcher on another build of the library (one without kmpgpu_set_headers included)"""
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


def gen_meta(n, seed=5):
    rng = np.random.default_rng(seed)
    meta = np.zeros(n, dtype=META_DTYPE)
    meta["src_ip"], meta["dst_ip"] = rng.choice(ADDR, n), rng.choice(ADDR, n)
    meta["src_port"], meta["dst_port"] = rng.choice(PORTS, n), rng.choice(PORTS, n)
    meta["proto"] = rng.choice([6, 17, 1], n)
    return meta


def gen_headers(n_hdr, seed=9):
    rng = np.random.default_rng(seed)
    h = np.zeros(n_hdr, dtype=HEADER_DTYPE)
    h["src_ip"], h["dst_ip"] = rng.choice(ADDR, n_hdr), rng.choice(ADDR, n_hdr)
    h["src_mask"], h["dst_mask"] = rng.choice(MASKS, n_hdr), rng.choice(MASKS, n_hdr)
    sp, dp = np.sort(rng.choice(PORTS, (n_hdr, 2)), axis=1), np.sort(rng.choice(PORTS, (n_hdr, 2)), axis=1)
    h["sport_lo"], h["sport_hi"], h["dport_lo"], h["dport_hi"] = sp[:, 0], sp[:, 1], dp[:, 0], dp[:, 1]
    h["len_lo"], h["len_hi"] = 0, 0xFFFFFFFF
    h["proto"] = rng.choice([6, 17, 1], n_hdr)
    h["flags"] = rng.integers(0, 4, n_hdr)
    return h


def row_of(meta, lens, h):
    """predicate h over all payloads, from the definition in include/kmpgpu.h"""
    s, d, sp, dp, pr = (meta[f].astype(np.int64) for f in ("src_ip", "dst_ip", "src_port", "dst_port", "proto"))

    def way(s, d, sp, dp):
        return (((s & int(h["src_mask"])) == (int(h["src_ip"]) & int(h["src_mask"]))) & ((d & int(h["dst_mask"])) == (int(h["dst_ip"]) & int(h["dst_mask"])))
                & (sp >= int(h["sport_lo"])) & (sp <= int(h["sport_hi"])) & (dp >= int(h["dport_lo"])) & (dp <= int(h["dport_hi"])))

    ok = (lens >= int(h["len_lo"])) & (lens <= int(h["len_hi"]))
    if not int(h["flags"]) & 1:
        ok &= pr == int(h["proto"])
    w = way(s, d, sp, dp)
    if int(h["flags"]) & 2:
        w |= way(d, s, dp, sp)
    return ok & w


def raw_headers(m, n_hdr, n):
    """(hdr_pkt_counts, rows as uint64[n_hdr, W]) of kmpgpu_scan_headers: the words as they come, not unpacked into a bool per payload"""
    W = (n + 63) // 64
    pc, hit_w = np.zeros(n_hdr, dtype=np.uint64), np.zeros((n_hdr, W), dtype=np.uint64)
    _lib.gpu_check(m._g.kmpgpu_scan_headers(m._ctx, pc.ctypes.data, None, hit_w.ctypes.data, None, None), "kmpgpu_scan_headers")
    return pc, hit_w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-this", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headers.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"header predicates (kmpgpu_set_headers), {n} x {L} B, medians of {args.reps} alternating rounds with min / quartiles / max, ms "
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
        line = f"(1) kmpgpu_scan_rules, {n_pat} tokens, {len(rules)} rules, no header predicates set: "
        if "a" in t:
            line += f"(a) parent {spread(t['a'])}, kernel_ms {statistics.median(own['a']):.3f}; "
        line += f"(b) this tree {spread(t['b'])}, kernel_ms {statistics.median(own['b']):.3f}"
        if "a" in t:
            mb = statistics.median(t["b"])
            line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
        say(line)
        # ---- (2) the header kernel
        meta = gen_meta(n)
        d_meta = torch.from_numpy(meta.view(np.uint8).reshape(-1).copy()).cuda()
        c.set_meta(d_meta)
        lens = np.full(n, L, dtype=np.int64)
        W2 = ((n + 63) // 64 + 1) & ~1
        for n_hdr in (1, 100, 1000):
            heads = gen_headers(n_hdr)
            c.set_headers(heads)
            pc, hit_w = raw_headers(c, n_hdr, n)
            for q in {0, n_hdr // 2, n_hdr - 1}:
                want = row_of(meta, lens, heads[q])
                assert np.array_equal(np.unpackbits(hit_w[q].view(np.uint8), bitorder="little")[:n].astype(bool), want) and int(pc[q]) == int(want.sum()), \
                    "the header kernel and the definition disagree"
            hit_share = float(pc.sum()) / n_hdr / n
            del hit_w
            tt, kk = [], []
            for rnd in range(3 + args.reps):
                c.profile_begin(64)
                dt, _ = timed(stream, lambda: c.scan_headers())
                prof = c.profile_end(64)
                if rnd >= 3:
                    tt.append(dt); kk.append(float(prof[-1]))
            moved = 20 * n + n_hdr * W2 * 8
            k_med = statistics.median(kk)
            say(f"(2) {n_hdr} predicates ({hit_share * 100:.1f} % of the payloads per predicate): kmpgpu_scan_headers {spread(tt)}; header kernel alone "
                f"{spread(kk)}; it must move 20 x {n} + {n_hdr} x {W2} x 8 = {moved} bytes: {moved / k_med / 1e6:.1f} GB/s, "
                f"{moved / (k_med * 1e-3) / HBM_PEAK * 100:.2f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM rate; "
                f"{k_med * 1e6 / n_hdr / n * 1e3:.2f} ps per (predicate, payload)")
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
