"""What the offset windows (kmpgpu_set_windows) cost kmpgpu_scan_packets (profiles/windows.txt).

    python3 tools/windows.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/windows.txt]
    rocprofv3 --kernel-trace --stats -- python3 tools/windows.py --reps 3        (where the time of a pass goes)

Shapes, all on 1 M x 1500 B payloads (the bench arena, synthetic S1), as tools/packets.py:
  needle   the 16-byte needle, planted in ~10 % of the payloads (flat streaming kernel);
  tokens   strings.txt's 97 tokens (fused pass);
  dense    one-letter text x a 16-byte pattern of that letter: every start offset matches.
Configurations, one context each on the same device arena, the calls alternating so that drift hits them alike:
  (a)      the parent commit's library (--parent-lib; left out without it);
  (b)      this tree's library, no windows;
  (c63)    this tree's library, the window [0, 63] on every pattern;
  (cmax)   this tree's library, the window [0, UINT32_MAX - 1] on every pattern: not the default, and always true -- the filter
           runs and drops nothing, so the outputs are those of (b).
Times are HIP events on the contexts' stream around each kmpgpu_scan_packets call (zeroing, scan launches, reduces, the small
downloads), medians of --reps calls after a warm-up; for (a) also the smallest and the largest, and the quartiles: the spread that
(b) is held against."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

U32_MAX = 0xFFFFFFFF


def matcher_on(path):
    """a GpuMatcher on another build of the library (one without kmpgpu_set_windows included)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows.txt"))
    args = ap.parse_args()
    n, L, stride = 1_000_000, 1500, 1504
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"kmpgpu_scan_packets with and without offset windows, {n} x {L} B, medians of {args.reps} alternating calls "
             f"(GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]
    shapes = [("needle", "needle, ~10 % of payloads (flat)", K.SynthParams.make(seed=1234, needle=needle, plant_permille=100), [needle]),
              ("tokens", "strings.txt x 97 (fused)", K.SynthParams.make(seed=1234, needle=needle, plant_permille=100), tokens),
              ("dense", "one-letter text x 'a' * 16 (flat, every offset matches)",
               K.SynthParams.make(seed=1234, needle=b"a", plant_permille=0, lo=ord("a"), span=1), [b"a" * 16])]
    ms = {"b": GpuMatcher(0), "c63": GpuMatcher(0), "cmax": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    try:
        for m in ms.values():
            m.set_stream(stream.cuda_stream)
        first = next(iter(ms.values()))
        first.fixed_index(d_off, d_len, L, 16)
        for key, name, sp, pats in shapes:
            first.synth_fill(d_arena, d_off, d_len, sp)
            first.sync()
            for m in ms.values():
                m.set_patterns(pats)
                m.attach_arena(d_arena, d_off, d_len)
            ms["c63"].set_windows([(0, 63)] * len(pats))
            ms["cmax"].set_windows([(0, U32_MAX - 1)] * len(pats))
            res = {c: m.scan_packets(hits=(key != "tokens")) for c, m in ms.items()}
            want = ms["b"].scan()[0].tolist()
            for c, r in res.items():                                     # the counts never follow the windows
                assert r["counts"].tolist() == want, c
            for c in ("a", "cmax"):                                      # no windows, and windows that drop nothing: the parent's outputs
                if c in res:
                    assert res[c]["pkt_counts"].tolist() == res["b"]["pkt_counts"].tolist() and (res[c]["any"] == res["b"]["any"]).all(), c
                    if "hits" in res["b"]:
                        assert (res[c]["hits"] == res["b"]["hits"]).all(), c
            assert (res["c63"]["pkt_counts"] <= res["b"]["pkt_counts"]).all()
            t = {c: [] for c in ms}
            own = {c: [] for c in ms}
            for _ in range(3):                                           # warm-up
                for m in ms.values():
                    m.scan_packets()
            for _ in range(args.reps):
                for c, m in ms.items():
                    dt, r = timed(stream, lambda: m.scan_packets())
                    t[c].append(dt)
                    own[c].append(r["timing"].kernel_ms)
            med = {c: statistics.median(v) for c, v in t.items()}
            line = (f"({key}) {name}: {len(pats)} patterns, {sum(want)} matches; payloads hit: no windows {int(res['b']['any'].sum())}, "
                    f"[0, 63] {int(res['c63']['any'].sum())}; packets call ms: ")
            line += ", ".join(f"({c}) {med[c]:.3f} (kernel_ms {statistics.median(own[c]):.3f})" for c in ms)
            if "a" in t:
                q = statistics.quantiles(t["a"], n=4)
                line += (f"; (a) min {min(t['a']):.3f} q1 {q[0]:.3f} q3 {q[2]:.3f} max {max(t['a']):.3f}; (b) / (a) {med['b'] / med['a']:.4f}")
            line += f"; (c63) / (b) {med['c63'] / med['b']:.4f}, (cmax) / (b) {med['cmax'] / med['b']:.4f}"
            lines.append(line)
            print(line, flush=True)
    finally:
        for m in ms.values():
            m.close()
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
