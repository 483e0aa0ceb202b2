"""The five compacting arena builders -- kmpgpu_load_selected, _decoded, _base64, _fields, _seams -- on this tree's library against the
parent commit's, after their kernels moved onto one skeleton (csrc/kmp_compact_dev.h; DESIGN.md, "The compacting skeleton";
profiles/compact.txt).

    python3 tools/compact.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 20] [--shapes 1500,64] [--out profiles/compact.txt]

1 000 000 payloads of 1500 B and of 64 B; the arenas are those of tools/decode.py, tools/base64_runs.py, tools/fields.py (1500 B only: its
request line does not fit 64) and the flows of tools/seams.py.  Per shape:
  load_selected   every bit set, the bitmap on the device
  load_decoded    percent, no '%' in the arena; one %2e per payload
  load_base64     min_run 16: no run of 16; one run of 24 per payload; the payload is one run
  load_fields     headers; body (a request with its blank line in the first 256 bytes)
  load_seams      reach 98 over 10 000 flows of Zipf sizes
Per case, first: the call once on either library, both results downloaded and required byte-equal -- arena, offsets and lengths.  Then (a)
the parent's library and (b) this tree's by turns inside each round, so that drift hits them alike, under kmpgpu_profile_begin .. _end:
kernel_ms of kmpgpu_last_timing as medians with min / quartiles / max of --reps repeats after a warm-up, and the median of every recorded
launch.  Unchanged: (b)'s median inside (a)'s min .. max of the same run."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import DECODE_PERCENT, FIELD_NAMES, GpuMatcher  # noqa: E402

import base64_runs  # noqa: E402  (tools/: the arenas of the loaders' own profiles)
import decode  # noqa: E402
import fields  # noqa: E402
from headers import matcher_on, spread  # noqa: E402  (tools/headers.py: the same instrument)
from seams import gen_flows, gen_meta  # noqa: E402

N = decode.N
MIN_RUN = base64_runs.MIN_RUN
REACH = 98
FLOWS = "10 000 flows, Zipf sizes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1500,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact.txt"))
    args = ap.parse_args()
    assert base64_runs.N == N
    srcs = {"a": matcher_on(args.parent_lib), "b": GpuMatcher(0)}
    dsts = {"a": matcher_on(args.parent_lib), "b": GpuMatcher(0)}
    lines = [f"the compacting arena builders, (a) the parent commit's library and (b) this tree's by turns, {N} payloads, kernel_ms, medians of "
             f"{args.reps} repeats with min / quartiles / max, ms, and the median of every launch (GPU: {torch.cuda.get_device_name(0)})"]
    outside = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def case(label, d_a, d_o, d_l, call, prepare=None):
        """call(dst, src): the loader on dst's library; returns nothing, asserts its own return code"""
        for key in "ab":
            srcs[key].attach_arena(d_a, d_o, d_l)
            if prepare:
                prepare(srcs[key])
        got = {}
        for key in "ab":
            call(dsts[key], srcs[key])
            got[key] = dsts[key].arena_download()
        assert all(np.array_equal(x, y) for x, y in zip(got["a"], got["b"])), f"{label}: the two libraries' arenas differ"
        n_dst, n_bytes = len(got["b"][1]), len(got["b"][0])
        del got
        t = {key: [] for key in "ab"}
        launches = {key: [] for key in "ab"}
        for rnd in range(3 + args.reps):
            for key in "ab":
                dsts[key].profile_begin(16)
                call(dsts[key], srcs[key])
                prof = [float(x) for x in dsts[key].profile_end(16)]
                if rnd >= 3:
                    t[key].append(dsts[key].last_timing().kernel_ms)
                    launches[key].append(prof)
        assert len({len(p) for key in "ab" for p in launches[key]}) == 1, f"{label}: the launch counts differ"
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        inside = min(t["a"]) <= mb <= max(t["a"])
        if not inside:
            outside.append(label)
        say(f"  {label}: {n_dst} payloads, {n_bytes} bytes, byte-equal")
        for key in "ab":
            say(f"    ({key}) kernel_ms {spread(t[key])}; launches "
                + " ".join(f"{statistics.median(p[i] for p in launches[key]):.3f}" for i in range(len(launches[key][0]))))
        say(f"    (b) / (a) {mb / ma:.4f}; (a)'s range {min(t['a']):.3f} .. {max(t['a']):.3f}, (b)'s median inside it: {'yes' if inside else 'NO'}")

    def selected(ones):
        def call(dst, src):
            n_out = C.c_uint64()
            assert dst._g.kmpgpu_load_selected(dst._ctx, src._ctx, ones.data_ptr(), 1, C.byref(n_out)) == 0 and n_out.value == N
        return call

    def decoded(dst, src):
        assert dst._g.kmpgpu_load_decoded(dst._ctx, src._ctx, DECODE_PERCENT, 0, None, None, None) == 0

    def base64(dst, src):
        assert dst._g.kmpgpu_load_base64(dst._ctx, src._ctx, MIN_RUN, 0, None, None, None) == 0

    def field(name):
        def call(dst, src):
            st = _lib.FieldsStats()
            assert dst._g.kmpgpu_load_fields(dst._ctx, src._ctx, FIELD_NAMES[name], 0, None, None, C.byref(st)) == 0 and st.n_present == N
        return call

    try:
        for L in [int(s) for s in args.shapes.split(",") if s]:
            off, ln, nbytes = K.arena_layout(None, L, N)
            d_o = torch.from_numpy(off.astype(np.int64)).cuda()
            d_l = torch.from_numpy(ln.astype(np.int32)).cuda()
            ones = torch.full(((N + 63) // 64,), -1, dtype=torch.int64, device="cuda")
            say(f"shape {L}: {N} payloads of {L} bytes, {nbytes} slot bytes")

            d_a = decode.make_arena(L, "none")
            assert d_a.numel() == nbytes
            torch.cuda.synchronize()
            case("load_selected, all bits", d_a, d_o, d_l, selected(ones))
            case("load_decoded, no escape", d_a, d_o, d_l, decoded)
            d_meta = torch.from_numpy(gen_meta(gen_flows(FLOWS, N)).view(np.uint8).reshape(-1).copy()).cuda()

            def flows(m):
                m.set_meta(d_meta)
                m.build_flows()

            case(f"load_seams, reach {REACH}, {FLOWS}", d_a, d_o, d_l, lambda dst, src: dst.load_seams(src, REACH), prepare=flows)
            del d_a, d_meta
            torch.cuda.empty_cache()
            d_a = decode.make_arena(L, "one %2e per payload")
            torch.cuda.synchronize()
            case("load_decoded, one %2e per payload", d_a, d_o, d_l, decoded)
            del d_a
            for run_case in base64_runs.CASES:
                torch.cuda.empty_cache()
                d_a = base64_runs.make_arena(L, run_case)
                torch.cuda.synchronize()
                case(f"load_base64, {run_case}", d_a, d_o, d_l, base64)
                del d_a
            if L == fields.L:
                torch.cuda.empty_cache()
                d_a = fields.make_arena(N, "blank line in the first 256 bytes")
                torch.cuda.synchronize()
                for name in ("headers", "body"):
                    case(f"load_fields, {name}", d_a, d_o, d_l, field(name), prepare=lambda m: m.http_locate())
                del d_a
            torch.cuda.empty_cache()
        say("every (b) median inside (a)'s range" if not outside else "outside (a)'s range: " + "; ".join(outside))
    finally:
        for m in list(dsts.values()) + list(srcs.values()):
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
