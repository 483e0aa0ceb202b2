"""What kmpgpu_load_base64 costs, kernel by kernel, against kmpgpu_load_decoded (percent, nothing to decode) and kmpgpu_load_selected
with all bits set on the same arenas, and the unchanged calls against the parent commit's library (profiles/base64.txt).

    python3 tools/base64_runs.py [--parent-lib <libkmpgpu.so of the parent commit>] [--reps 20] [--shapes 1500,64] [--out profiles/base64.txt]

Shapes: 1 M x 1500 B and 1 M x 64 B.  Cases: no run of min_run = 16 at all (lower-case words of seven letters and a blank); one
24-character run per payload (at byte 5); a payload that is one run.  Per shape and case, by turns inside each round so that drift hits
them alike:
  (a)  kmpgpu_load_base64 (min_run 16, no flags) under kmpgpu_profile_begin .. _end: the four recorded spans -- lengths, the two scan
       kernels, index, write -- and kernel_ms of kmpgpu_last_timing;
  (b)  kmpgpu_load_decoded (percent, no flags) over the same arena, which holds no '%': its copy path, the same spans;
  (c)  kmpgpu_load_selected with every bit set, the bitmap on the device: kernel_ms of kmpgpu_last_timing.
  (3)  with --parent-lib: kmpgpu_scan_rules and kmpgpu_load_decoded over the first arena, (a) on the parent's library, (b) on this tree's;
       unchanged: (b)'s median inside (a)'s own range of the run.
Medians with min / quartiles / max of --reps repeats after a warm-up."""
import argparse
import ctypes as C
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
from multithreading_string_matching_amd.matcher import DECODE_PERCENT, GpuMatcher  # noqa: E402

from headers import gen_rules, matcher_on, spread  # noqa: E402  (tools/headers.py: the same instrument)

N = 1_000_000
MIN_RUN = 16
CASES = ["no run of 16", "one run of 24 per payload", "the payload is one run"]
SPANS = ["lengths", "scan x 2", "index", "write"]
RUN24 = b"QUJDREVGR0hJSktMTU5PUFFS"


def make_arena(L, case):
    """N payloads of L bytes in slots of round_up(L, 16), padding 0x00, and the 64 bytes K.arena_layout leaves behind them, on the device"""
    slot = max(16, (L + 15) // 16 * 16)
    g = torch.Generator(device="cuda")
    g.manual_seed(L)
    a = torch.randint(97, 123, (N, slot), dtype=torch.uint8, device="cuda", generator=g)
    if case != "the payload is one run":
        a[:, 7::8] = 0x20
    if case == "one run of 24 per payload":
        a[:, 4] = 0x20
        a[:, 5:29] = torch.tensor(list(RUN24), dtype=torch.uint8, device="cuda")
        a[:, 29] = 0x20
    a[:, L:] = 0
    return torch.cat([a.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1500,64")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "base64.txt"))
    args = ap.parse_args()
    src, dst, dec, sel = GpuMatcher(0), GpuMatcher(0), GpuMatcher(0), GpuMatcher(0)
    g = dst._g
    lines = [f"kmpgpu_load_base64 (min_run {MIN_RUN}) against kmpgpu_load_decoded (percent, no '%' in the arena) and kmpgpu_load_selected (all bits), "
             f"{N} payloads, kernel_ms, medians of {args.reps} repeats by turns with min / quartiles / max, ms (GPU: {torch.cuda.get_device_name(0)}); "
             f"parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def by_turns(calls, reps=args.reps):
        t = {key: [] for key in calls}
        for rnd in range(3 + reps):
            for key, fn in calls.items():
                x = fn()
                if rnd >= 3:
                    t[key].append(x)
        return t

    try:
        first = None
        for L in [int(s) for s in args.shapes.split(",") if s]:
            off, ln, nbytes = K.arena_layout(None, L, N)
            d_o = torch.from_numpy(off.astype(np.int64)).cuda()
            d_l = torch.from_numpy(ln.astype(np.int32)).cuda()
            ones = torch.full(((N + 63) // 64,), -1, dtype=torch.int64, device="cuda")
            say(f"shape {L}: {N} payloads of {L} bytes, {nbytes} slot bytes")
            for case in CASES:
                d_a = make_arena(L, case)
                assert d_a.numel() == nbytes
                torch.cuda.synchronize()
                src.attach_arena(d_a, d_o, d_l)
                st, st_d = _lib.DecodeStats(), _lib.DecodeStats()
                n_out = C.c_uint64()
                spans = {"a": [[] for _ in SPANS], "b": [[] for _ in SPANS]}

                def call_a():
                    dst.profile_begin(8)
                    rc = g.kmpgpu_load_base64(dst._ctx, src._ctx, MIN_RUN, 0, None, None, C.byref(st))
                    for i, x in enumerate(dst.profile_end(8)):
                        spans["a"][i].append(float(x))
                    assert rc == 0 and st.n_payloads == N
                    return dst.last_timing().kernel_ms

                def call_b():
                    dec.profile_begin(8)
                    rc = g.kmpgpu_load_decoded(dec._ctx, src._ctx, DECODE_PERCENT, 0, None, None, C.byref(st_d))
                    for i, x in enumerate(dec.profile_end(8)):
                        spans["b"][i].append(float(x))
                    assert rc == 0 and st_d.n_payloads == N and st_d.n_changed == 0
                    return dec.last_timing().kernel_ms

                def call_c():
                    assert g.kmpgpu_load_selected(sel._ctx, src._ctx, ones.data_ptr(), 1, C.byref(n_out)) == 0 and n_out.value == N
                    return sel.last_timing().kernel_ms

                t = by_turns({"a": call_a, "b": call_b, "c": call_c})
                ma, mb, mc = (statistics.median(t[k]) for k in "abc")
                moved = int(st.bytes_in) * 2 + int(st.bytes_out)
                say(f"  {case}: {int(st.n_changed)} payloads changed, {int(st.bytes_in)} -> {int(st.bytes_out)} bytes")
                say(f"    (a) load_base64 kernel_ms {spread(t['a'])} ({moved / ma / 1e6:.0f} GB/s over two reads and one write); "
                    + ", ".join(f"{name} {statistics.median(v[-args.reps:]):.3f}" for name, v in zip(SPANS, spans["a"])))
                say(f"    (b) load_decoded kernel_ms {spread(t['b'])}; "
                    + ", ".join(f"{name} {statistics.median(v[-args.reps:]):.3f}" for name, v in zip(SPANS, spans["b"])))
                say(f"    (c) load_selected kernel_ms {spread(t['c'])}; (a) / (b) {ma / mb:.3f}, (a) / (c) {ma / mc:.3f}; (b)'s range {min(t['b']):.3f} .. "
                    f"{max(t['b']):.3f}, (a)'s median inside it: {'yes' if min(t['b']) <= ma <= max(t['b']) else 'NO'}")
                if first is None:
                    first = (d_a, d_o, d_l)
                else:
                    del d_a
                src.attach_arena(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"),
                                 torch.zeros(0, dtype=torch.int32, device="cuda"))
                torch.cuda.empty_cache()

        if args.parent_lib and first is not None:
            parent = matcher_on(args.parent_lib)
            tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
            rules = gen_rules(random.Random(100), 100, len(tokens))
            ms = {"a": parent, "b": src}
            for m in ms.values():
                m.set_patterns(tokens)
                m.attach_arena(*first)
                m.set_rules(rules)
            res = {key: m.scan_rules(hits=True) for key, m in ms.items()}
            assert all(np.array_equal(res["a"][k], res["b"][k]) for k in ("hits", "any", "counts", "rule_pkt_counts"))

            def compare(label, calls):
                t = by_turns(calls)
                ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
                say(f"(3) {label}: (a) parent {spread(t['a'])}; (b) this tree {spread(t['b'])}; (b) / (a) {mb / ma:.4f}; the parent's range "
                    f"{min(t['a']):.3f} .. {max(t['a']):.3f}, (b)'s median inside it: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}")

            compare(f"kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules", {key: (lambda m=m: m.scan_rules()["timing"].kernel_ms) for key, m in ms.items()})
            dsts = {"a": matcher_on(args.parent_lib), "b": dst}

            def decoded(key):
                d = dsts[key]
                assert d._g.kmpgpu_load_decoded(d._ctx, ms[key]._ctx, DECODE_PERCENT, 0, None, None, None) == 0
                return d.last_timing().kernel_ms

            compare("kmpgpu_load_decoded", {key: (lambda key=key: decoded(key)) for key in ms})
            assert all(np.array_equal(x, y) for x, y in zip(dsts["a"].arena_download(), dsts["b"].arena_download()))
            dsts["a"].close()
            parent.close()
    finally:
        for m in (src, dst, dec, sel):
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
