"""kmpgpu_scan_alerts + kmpgpu_alerts_read against the route a caller had before them: the family's call with the bit matrix
downloaded, then a walk of it on the host (profiles/alerts.txt).

    python3 tools/alerts.py [--parent-lib <libkmpgpu.so of the parent commit>] [--reps 20] [--out profiles/alerts.txt]

Shapes, all on 1 M x 1500 B payloads (the bench arena, synthetic S1), the rule sets those of tools/rules.py:
  (p) strings.txt's 97 tokens, the patterns family;
  (a) the 97 tokens with 100 generated rules, the rules family;
  (b) 1 000 random patterns of 4..12 bytes with 1 000 generated rules, the rules family.
Times are medians of --reps calls after a warm-up; the two routes alternate, so that drift hits them alike.
  list route    host clock around scan_alerts(UINT64_MAX) and alerts_read of all records;
  matrix route  host clock around kmpgpu_scan_packets / kmpgpu_scan_rules with hits_out and the host walk.  The walk: numpy
                unpackbits (little-endian bit order) of the rows x W words, transposed, np.nonzero -- which gives the pairs sorted
                by payload, then row, the list's order; the two lists are compared once, exactly;
  kernels       kmp_alerts_count_kernel, the two scan kernels and kmp_alerts_fill_kernel, recorded by kmpgpu_profile_begin / _end
                (the last three entries of the pass), and for the patterns family next to kmp_marks_reduce_kernel over the same
                matrix (the entry in front of them), which reads it once, coalesced: what one read of it costs.  (The rule rows have
                no such reader: the rules kernel writes them.)  The matrix route is timed min(--reps, 5) times: its walk of the
                1 000-row matrix takes seconds.
With --parent-lib: kmpgpu_scan_packets and kmpgpu_scan_rules of the parent build before and after this build's, in the same run, HIP
events around each call: this build's median has to lie inside the spread of the parent's two medians' samples."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from rules import gen_rules  # noqa: E402
from windows import matcher_on, timed  # noqa: E402


def host_walk(words, n):
    """the pairs (payload, row) of the set bits of uint64[rows, W], sorted by payload, then row"""
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n]
    k, i = np.nonzero(bits.T)
    return k, i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alerts.txt"))
    args = ap.parse_args()
    n, L, stride = 1_000_000, 1500, 1504
    W = (n + 63) // 64
    W2 = (W + 1) // 2 * 2
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    rng = random.Random(1000)
    rand1000 = [bytes(rng.randrange(ord("a"), ord("z") + 1) for _ in range(rng.randrange(4, 13))) for _ in range(1000)]
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    g = _lib.gpu_lib()
    med = statistics.median
    lines = [f"kmpgpu_scan_alerts + kmpgpu_alerts_read vs the family's call with hits_out + a numpy walk (unpackbits, nonzero), {n} x {L} B, "
             f"medians of {args.reps} (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]
    shapes = [("p", "strings.txt x 97, patterns family", tokens, 0, "patterns"), ("a", "strings.txt x 97, 100 rules", tokens, 100, "rules"),
              ("b", "1000 random 4..12-byte patterns, 1000 rules", rand1000, 1000, "rules")]
    sp = K.SynthParams.make(seed=1234, needle=needle, plant_permille=100)
    ms = {"new": GpuMatcher(0)}
    if args.parent_lib:
        ms["parent"] = matcher_on(args.parent_lib)
    try:
        for m in ms.values():
            m.set_stream(stream.cuda_stream)
        m = ms["new"]
        m.fixed_index(d_off, d_len, L, 16)
        m.synth_fill(d_arena, d_off, d_len, sp)
        m.sync()
        for key, name, pats, n_rules, family in shapes:
            n_pat = len(pats)
            rules = gen_rules(random.Random(n_rules), n_rules, n_pat) if n_rules else []
            rows = n_rules if family == "rules" else n_pat
            for x in ms.values():
                x.set_patterns(pats)
                x.attach_arena(d_arena, d_off, d_len)
                if rules:
                    x.set_rules(rules)
            words = np.zeros((rows, W), dtype=np.uint64)
            sibling = g.kmpgpu_scan_rules if family == "rules" else g.kmpgpu_scan_packets

            def matrix_route():
                assert sibling(m._ctx, None, None, words.ctypes.data, None, None) == 0
                return host_walk(words, n)

            def list_route():
                return m.scan_alerts(family)

            k, i = matrix_route()
            res = list_route()
            assert res["n_found"] == k.size and np.array_equal(res["alerts"]["packet"], k.astype(np.uint64))
            assert np.array_equal(res["alerts"]["index"], i.astype(np.uint32))

            def profiled():
                m.profile_begin(64)
                r = m.scan_alerts(family, read=False)
                return m.profile_end(64), r["timing"]

            for _ in range(2):                                       # warm-up
                list_route(); profiled()
            t_list, t_mat, k_ms, cnt, scn, fil, red = [], [], [], [], [], [], []
            for rep in range(args.reps):
                t0 = time.perf_counter()
                list_route()
                t_list.append((time.perf_counter() - t0) * 1e3)
                if rep < 5:
                    t0 = time.perf_counter()
                    matrix_route()
                    t_mat.append((time.perf_counter() - t0) * 1e3)
                p, t = profiled()
                k_ms.append(t.kernel_ms); cnt.append(float(p[-3])); scn.append(float(p[-2])); fil.append(float(p[-1]))
                if family == "patterns":
                    red.append(float(p[-4]))
            mat_bytes = rows * W2 * 8
            line = (f"({key}) {name}: {rows} rows, {res['n_found']} records on {res['n_packets']} payloads ({res['n_found'] * 16 / 1e6:.2f} MB of records, "
                    f"{rows * W * 8 / 1e6:.1f} MB of matrix); list route {med(t_list):.3f} ms, matrix route {med(t_mat):.3f} ms: {med(t_mat) / med(t_list):.1f}x; "
                    f"alerts pass kernel_ms {med(k_ms):.3f}; count {med(cnt) * 1e3:.1f} us ({mat_bytes / med(cnt) / 1e6:.0f} GB/s of matrix), "
                    f"scan {med(scn) * 1e3:.1f} us, fill {med(fil) * 1e3:.1f} us")
            if red:
                line += f"; kmp_marks_reduce_kernel on the same matrix {med(red) * 1e3:.1f} us ({mat_bytes / med(red) / 1e6:.0f} GB/s)"
            lines.append(line)
            print(line, flush=True)
            if "parent" in ms:
                for call in (["scan_packets", "scan_rules"] if rules else ["scan_packets"]):
                    t = {"parent before": [], "new": [], "parent after": []}
                    for c, x in (("parent before", ms["parent"]), ("new", m), ("parent after", ms["parent"])):
                        for _ in range(3):
                            getattr(x, call)()
                        for _ in range(args.reps):
                            t[c].append(timed(stream, getattr(x, call))[0])
                    pa = t["parent before"] + t["parent after"]
                    inside = min(pa) <= med(t["new"]) <= max(pa)
                    line = (f"    {call}: parent before {med(t['parent before']):.3f} ms, this build {med(t['new']):.3f} ms, parent after "
                            f"{med(t['parent after']):.3f} ms; the parent's samples span {min(pa):.3f} .. {max(pa):.3f} ms: this build's median "
                            f"{'inside' if inside else 'OUTSIDE'}")
                    lines.append(line)
                    print(line, flush=True)
    finally:
        for x in ms.values():
            x.close()
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
