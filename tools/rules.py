"""kmpgpu_scan_rules against the route a caller had before it: kmpgpu_scan_packets with hits_out, then the rules applied to
the packed words on the host with numpy (profiles/rules.txt).

    python3 tools/rules.py [--reps 30] [--out profiles/rules.txt]

Shapes, both on 1 M x 1500 B payloads (the bench arena, synthetic S1):
  (a) strings.txt's 97 tokens with 100 generated rules of 1..4 terms;
  (b) 1 000 random patterns of 4..12 bytes with 1 000 generated rules of 1..4 terms.
Times are medians of --reps calls after a warm-up; the two routes alternate, so that drift hits them alike.
  end to end   host clock around the synchronous call (and, for the old route, the numpy pass behind it): what a caller waits;
  device       HIP events on the context's stream around kmpgpu_scan_rules, and the call's own kernel_ms;
  rules kernel its launch alone, recorded by kmpgpu_profile_begin / _end (the last launch of the call), over the bytes it
               moves at most: (sum of terms + n_rules) x W2 x 8, W2 = the words of a row on the device;
  marks reduce kmp_marks_reduce_kernel on the same matrix, as a reference point for a kernel of that shape: kernel_ms of
               kmpgpu_scan_packets minus what kmpgpu_scan_rules spends in front of its rules kernel, over n_pat x W2 x 8."""
import argparse
import ctypes as C
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


def popcount(a):
    if hasattr(np, "bitwise_count"):
        return int(np.bitwise_count(a).sum())
    return int(np.unpackbits(a.view(np.uint8)).sum())


def host_rules(hit_words, rules, tail):
    """the rules over the packed rows of kmpgpu_scan_packets: (rule_pkt_counts, any words)"""
    any_w = np.zeros(hit_words.shape[1], dtype=np.uint64)
    counts = np.zeros(len(rules), dtype=np.uint64)
    for r, (pos, neg) in enumerate(rules):
        if pos:
            acc = hit_words[pos[0]].copy()
            for i in pos[1:]:
                acc &= hit_words[i]
        else:
            acc = np.full(hit_words.shape[1], ~np.uint64(0), dtype=np.uint64)
            acc[-1] = tail
        for i in neg:
            acc &= ~hit_words[i]
        counts[r] = popcount(acc)
        any_w |= acc
    return counts, any_w


def gen_rules(rng, n_rules, n_pat):
    rules = []
    for _ in range(n_rules):
        pos, neg = [], []
        for _ in range(rng.randrange(1, 5)):
            (neg if rng.random() < 0.25 else pos).append(rng.randrange(n_pat))
        rules.append((pos, neg))
    return rules


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    r = fn()
    wall = (time.perf_counter() - t0) * 1e3
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), wall, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rules.txt"))
    args = ap.parse_args()
    n, L, stride = 1_000_000, 1500, 1504
    W = (n + 63) // 64
    W2 = (W + 1) // 2 * 2
    tail = np.uint64((1 << (n % 64)) - 1) if n % 64 else ~np.uint64(0)
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    rng = random.Random(1000)
    rand1000 = [bytes(rng.randrange(ord("a"), ord("z") + 1) for _ in range(rng.randrange(4, 13))) for _ in range(1000)]
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    g = _lib.gpu_lib()
    lines = [f"kmpgpu_scan_rules vs kmpgpu_scan_packets(hits_out) + the rules on the host (numpy), {n} x {L} B, medians of {args.reps} "
             f"(GPU: {torch.cuda.get_device_name(0)})"]
    shapes = [("a", "strings.txt x 97, 100 rules", tokens, 100), ("b", "1000 random 4..12-byte patterns, 1000 rules", rand1000, 1000)]
    sp = K.SynthParams.make(seed=1234, needle=needle, plant_permille=100)
    with GpuMatcher(0) as m:
        m.set_stream(stream.cuda_stream)
        m.fixed_index(d_off, d_len, L, 16)
        m.synth_fill(d_arena, d_off, d_len, sp)
        m.sync()
        for key, name, pats, n_rules in shapes:
            n_pat = len(pats)
            rules = gen_rules(random.Random(n_rules), n_rules, n_pat)
            n_terms = sum(len(a) + len(b) for a, b in rules)
            m.set_patterns(pats)
            m.attach_arena(d_arena, d_off, d_len)
            m.set_rules(rules)
            hit_words = np.zeros((n_pat, W), dtype=np.uint64)
            t_pk = _lib.Timing()

            def old_route():
                gpu_rc = g.kmpgpu_scan_packets(m._ctx, None, None, hit_words.ctypes.data, None, C.byref(t_pk))
                assert gpu_rc == 0
                return host_rules(hit_words, rules, tail)

            rc_buf, any_buf, cnt_buf = np.zeros(n_rules, np.uint64), np.zeros(W, np.uint64), np.zeros(n_pat, np.uint64)
            t_new = _lib.Timing()

            def new_route():
                assert g.kmpgpu_scan_rules(m._ctx, rc_buf.ctypes.data, any_buf.ctypes.data, None, cnt_buf.ctypes.data, C.byref(t_new)) == 0
                return t_new.kernel_ms

            def packets_only():
                assert g.kmpgpu_scan_packets(m._ctx, None, None, None, None, C.byref(t_pk)) == 0
                return t_pk.kernel_ms

            def rules_kernel_ms():
                m.profile_begin(64)
                k_ms = new_route()
                ms = m.profile_end(64)
                assert 2 <= len(ms) < 64                                # scan launches, then the rules kernel
                return float(ms[-1]), k_ms

            want_counts, want_any = old_route()
            res = m.scan_rules()
            assert res["rule_pkt_counts"].tolist() == want_counts.tolist()
            any_bits = np.concatenate([res["any"], np.zeros(W * 64 - n, dtype=bool)])
            assert np.array_equal(np.packbits(any_bits, bitorder="little").view(np.uint64), want_any)
            assert res["counts"].tolist() == m.scan()[0].tolist()
            new_route()
            assert rc_buf.tolist() == want_counts.tolist() and np.array_equal(any_buf, want_any)
            for _ in range(3):                                       # warm-up
                new_route(); old_route(); packets_only(); rules_kernel_ms()
            new_dev, new_wall, new_k, old_wall, old_pk_wall, pk_k, rk, rk_call = [], [], [], [], [], [], [], []
            for _ in range(args.reps):
                dev, wall, k_ms = timed(stream, new_route)
                new_dev.append(dev); new_wall.append(wall); new_k.append(k_ms)
                t0 = time.perf_counter()
                old_route()
                old_wall.append((time.perf_counter() - t0) * 1e3)
                old_pk_wall.append(t_pk.kernel_ms + t_pk.d2h_ms)
                pk_k.append(packets_only())
                a, b = rules_kernel_ms()
                rk.append(a); rk_call.append(b)
            med = statistics.median
            rules_ms = med(rk)
            front_ms = med(rk_call) - rules_ms                       # zeroing + scan launches of the marking pass
            reduce_ms = med(pk_k) - front_ms
            rules_bytes = (n_terms + n_rules) * W2 * 8
            reduce_bytes = n_pat * W2 * 8
            lines.append(
                f"({key}) {name}: {n_pat} patterns, {n_rules} rules of {n_terms} terms, {int(res['any'].sum())} payloads alerted; "
                f"end to end: scan_rules {med(new_wall):.3f} ms (device events {med(new_dev):.3f} ms, kernel_ms {med(new_k):.3f}), "
                f"scan_packets(hits_out) + numpy {med(old_wall):.3f} ms (of which pass + D2H of the {n_pat * W * 8 / 1e6:.1f} MB matrix "
                f"{med(old_pk_wall):.3f} ms); old / new {med(old_wall) / med(new_wall):.1f}x")
            lines.append(
                f"    rules kernel {rules_ms * 1e3:.1f} us = {100 * rules_ms / med(rk_call):.1f} % of the pass's kernel_ms, at most "
                f"{rules_bytes / 1e6:.1f} MB moved: {rules_bytes / rules_ms / 1e6:.0f} GB/s; "
                f"kmp_marks_reduce_kernel on the same matrix (by difference) {reduce_ms * 1e3:.1f} us, {reduce_bytes / 1e6:.1f} MB: "
                f"{reduce_bytes / max(reduce_ms, 1e-6) / 1e6:.0f} GB/s")
            print(lines[-2], flush=True)
            print(lines[-1], flush=True)
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
