"""What the HTTP field buffers cost: kmpgpu_http_locate against the pass that reads every byte once, kmpgpu_load_fields against
kmpgpu_load_selected with all bits set, and the unchanged calls against the parent commit's library (DESIGN.md §3.29;
profiles/fields.txt).

    python3 tools/fields.py [--parent-lib <libkmpgpu.so of the parent commit>] [--reps 20] [--out profiles/fields.txt]

1 M payloads of 1500 bytes, lower-case letters, kernel_ms of kmpgpu_last_timing unless said otherwise, medians of --reps repeats after a
warm-up, the calls of a section taking turns inside each round so that drift hits them alike.
  (1) the locate       three arenas: (a) no payload is HTTP; (b) every payload is a request whose blank line lies in the first 256 bytes;
                       (c) every payload is a request without a blank line.  The arena is attached anew before every call, which drops
                       the spans.  The yardstick, in the same rounds: kmp_decode_lengths_kernel over the same arena (the first span of
                       kmpgpu_load_decoded under kmpgpu_profile_begin .. _end), which reads every byte once.
  (2) the load         kmpgpu_load_fields over arena (b) with valid spans, for raw_uri (tens of bytes), headers and body (most of the
                       payload, from an odd offset), against kmpgpu_load_selected of all payloads in the same rounds.
  (3) unchanged calls  kmpgpu_scan_rules (strings.txt's tokens, 100 generated rules) and kmpgpu_load_decoded over arena (b): (a) the
                       parent's library, (b) this tree's; unchanged: (b)'s median inside (a)'s own range of the run.  Left out without
                       --parent-lib."""
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
from multithreading_string_matching_amd.matcher import DECODE_PERCENT, FIELD_NAMES, GpuMatcher  # noqa: E402

from headers import gen_rules, matcher_on, spread  # noqa: E402  (tools/headers.py: the same instrument)

L = 1500
REQUEST = b"GET /index.html?id=0123456789abcdef&x=%2e%2e HTTP/1.1\r\nHost: example\r\nUser-Agent: "
BLANK_AT = 199                  # "\r\n\r\n" from here in arena (b): the body starts at byte 203


def make_arena(n, kind):
    slot = (L + 15) // 16 * 16
    g = torch.Generator(device="cuda")
    g.manual_seed(len(kind))
    a = torch.randint(97, 123, (n, slot), dtype=torch.uint8, device="cuda", generator=g)
    a[:, L:] = 0
    if kind != "no HTTP":
        a[:, :len(REQUEST)] = torch.tensor(list(REQUEST), dtype=torch.uint8, device="cuda")
    if kind == "blank line in the first 256 bytes":
        a[:, BLANK_AT:BLANK_AT + 4] = torch.tensor(list(b"\r\n\r\n"), dtype=torch.uint8, device="cuda")
    return torch.cat([a.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields.txt"))
    args = ap.parse_args()
    n = args.payloads
    off, ln, nbytes = K.arena_layout(None, L, n)
    d_o = torch.from_numpy(off.astype(np.int64)).cuda()
    d_l = torch.from_numpy(ln.astype(np.int32)).cuda()
    ones = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    lines = [f"HTTP field buffers (kmpgpu_http_locate, kmpgpu_load_fields), {n} x {L} B, kernel_ms, medians of {args.reps} alternating repeats with "
             f"min / quartiles / max, ms (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def by_turns(calls, reps=args.reps):
        t = {key: [] for key in calls}
        for rnd in range(3 + reps):
            for key, fn in calls.items():
                x = fn()
                if rnd >= 3:
                    t[key].append(x)
        return t

    src, dst, sel = GpuMatcher(0), GpuMatcher(0), GpuMatcher(0)
    parent = matcher_on(args.parent_lib) if args.parent_lib else None
    g = dst._g
    try:
        arenas = {}
        for kind in ("no HTTP", "blank line in the first 256 bytes", "no blank line"):
            d_a = arenas[kind] = make_arena(n, kind)
            assert d_a.numel() == nbytes
            torch.cuda.synchronize()

            def locate():
                src.attach_arena(d_a, d_o, d_l)                      # drops the spans
                st = src.http_locate()
                t = src.last_timing()
                assert t.launches == 1
                return t.kernel_ms, st

            def lengths():
                dst.profile_begin(8)
                assert g.kmpgpu_load_decoded(dst._ctx, src._ctx, DECODE_PERCENT, 0, None, None, None) == 0
                return float(dst.profile_end(8)[0])

            _, st = locate()
            t = by_turns({"locate": lambda: locate()[0], "decode lengths": lengths})
            ml, md = statistics.median(t["locate"]), statistics.median(t["decode lengths"])
            say(f"(1) {kind}: {st['n_requests']} requests, {st['n_blank']} with a blank line, {st['bytes_scanned']} of {n * L} bytes scanned; "
                f"kmp_http_locate_kernel {spread(t['locate'])} ({st['bytes_scanned'] / ml / 1e6:.0f} GB/s of the bytes scanned); "
                f"kmp_decode_lengths_kernel {spread(t['decode lengths'])} ({n * L / md / 1e6:.0f} GB/s); locate / lengths {ml / md:.3f}")

        d_a = arenas["blank line in the first 256 bytes"]
        src.attach_arena(d_a, d_o, d_l)
        src.http_locate()
        n_out = C.c_uint64()
        fst = _lib.FieldsStats()

        def fields(name):
            assert g.kmpgpu_load_fields(dst._ctx, src._ctx, FIELD_NAMES[name], 0, None, None, C.byref(fst)) == 0 and fst.n_present == n
            t = dst.last_timing()
            assert t.launches == 5
            return t.kernel_ms

        def selected():
            assert g.kmpgpu_load_selected(sel._ctx, src._ctx, ones.data_ptr(), 1, C.byref(n_out)) == 0 and n_out.value == n
            return sel.last_timing().kernel_ms

        t = by_turns({"raw_uri": lambda: fields("raw_uri"), "headers": lambda: fields("headers"), "body": lambda: fields("body"), "load_selected": selected})
        ms_ = statistics.median(t["load_selected"])
        for name in ("raw_uri", "headers", "body"):
            fields(name)
            say(f"(2) kmpgpu_load_fields {name}: {int(fst.bytes_out)} field bytes of {int(fst.bytes_in)}; kernel_ms {spread(t[name])}; "
                f"/ load_selected {statistics.median(t[name]) / ms_:.3f}")
        say(f"(2) kmpgpu_load_selected, all {n} payloads: kernel_ms {spread(t['load_selected'])} ({2 * n * L / ms_ / 1e6:.0f} GB/s over one read and one write)")

        if parent is not None:
            tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
            rules = gen_rules(random.Random(100), 100, len(tokens))
            ms = {"a": parent, "b": src}
            for m in ms.values():
                m.set_patterns(tokens)
                m.attach_arena(d_a, d_o, d_l)
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
    finally:
        for m in (src, dst, sel, parent):
            if m is not None:
                m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
