"""Whole-payload passes (KMPGPU_OPT_WHOLE_PAYLOAD = 1) against the default strlen() rule, on the four benchmark shapes (DESIGN.md,
"Whole payloads"; profiles/whole_payload.txt).

    python3 tools/whole_payload.py [--reps 7] [--passes 60] [--default-only]

NUL-free input, where both rules give the same counts (checked before anything is timed):
    flat      1 M x 1500 B, one 16-byte needle             (kmp_scan_flat_kernel / kmp_scan_flat_whole_kernel)
    packed    1 M x 64..9000 B Zipf(1.1), the same needle  (kmp_scan_packed_kernel / ..._whole_kernel)
    fused     1 M x 1500 B x strings.txt (97 tokens)       (kmp_scan_multi_wide_kernel / ..._whole_wide_kernel: 1-byte tokens ride along)
    fused64   12 M x 64 B x strings.txt
NUL-laden input (no bar: the default rule legitimately skips work there, the whole-payload pass cannot): the flat and the fused
shape with a 0x00 in byte 3 of every payload (the DNS shape) and with 0x00 sprinkled at p = 1e-3 per byte.

A repeat = `passes` back-to-back enqueued passes after a settle-in, timed the two ways bench.py times its steps: the scan launches by
device events (kmpgpu_profile_begin / _end: "kernel"), and host clock over the enqueue loop and the final synchronise ("step").  The
repeats of option 0 and option 1 alternate in one process, so that drift hits both alike; min / median / max over the repeats.
--default-only times option 0 alone and never names the option: the form that also runs on a build that does not have it (the
parent commit, for the comparison in the same GPU call)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

OPT_WHOLE = 9
NEEDLE = b"NEEDLE_16B_PATRN"


def zipf_lengths(n, seed=4):
    rng = np.random.default_rng(seed)
    ranks = np.arange(1, 9000 - 64 + 2)
    p = 1.0 / ranks ** 1.1
    p /= p.sum()
    return (64 + rng.choice(len(ranks), size=n, p=p)).astype(np.uint32)


def device_arena(m, lens, fixed_len, n, sp):
    off, ln, nbytes = K.arena_layout(lens, fixed_len, n)
    d_a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_o = torch.from_numpy(off.astype(np.int64)).cuda()
    d_l = torch.from_numpy(ln.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    m.synth_fill(d_a, d_o, d_l, sp)
    m.sync()
    return d_a, d_o, d_l, int(ln.astype(np.int64).sum())


def timed(m, passes):
    m.sync()
    m.profile_begin(passes * 8)
    t0 = time.perf_counter()
    for _ in range(passes):
        m.scan_enqueue()
    m.sync()
    t1 = time.perf_counter()
    ms = m.profile_end(passes * 8)
    return float(ms.sum()) / passes * 1e3, (t1 - t0) / passes * 1e6            # us per pass: kernels, step


def fmt(xs):
    return f"{min(xs):8.1f} / {statistics.median(xs):8.1f} / {max(xs):8.1f}"


def leg(m, name, payload_bytes, args, same_counts):
    modes = (0,) if args.default_only else (0, 1)
    counts = {}
    for opt in modes:
        if not args.default_only:
            m.set_option(OPT_WHOLE, opt)
        counts[opt] = m.scan()[0].tolist()
    if not args.default_only:
        if same_counts:
            assert counts[0] == counts[1], (name, "the two rules differ on NUL-free input")
        else:
            assert counts[0] != counts[1] and all(a <= b for a, b in zip(counts[0], counts[1])), name
    for _ in range(args.settle):
        m.scan_enqueue()
    m.sync()
    kern = {o: [] for o in modes}
    step = {o: [] for o in modes}
    for _ in range(args.reps):
        for opt in modes:
            if not args.default_only:
                m.set_option(OPT_WHOLE, opt)
            for _ in range(10):
                m.scan_enqueue()
            k, s = timed(m, args.passes)
            kern[opt].append(k)
            step[opt].append(s)
    for opt in modes:
        med = statistics.median(kern[opt])
        print(f"{name:34s} option {opt}: kernel us min/med/max {fmt(kern[opt])}   step us {fmt(step[opt])}   "
              f"{payload_bytes / med / 1e3:7.0f} GB/s   matches {sum(counts[opt])}", flush=True)
    if not args.default_only:
        a, b = statistics.median(kern[0]), statistics.median(kern[1])
        print(f"{name:34s} whole / default (median kernel): {b / a:.4f}; spread of the default's repeats: +-{(max(kern[0]) - min(kern[0])) / 2 / a * 100:.2f} %",
              flush=True)
        m.set_option(OPT_WHOLE, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=60)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--default-only", action="store_true")
    args = ap.parse_args()
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    print(f"tools/whole_payload.py: {args.reps} repeats of {args.passes} passes per configuration and option"
          + (" (default rule only)" if args.default_only else ", option 0 = strlen rule, 1 = whole payloads"), flush=True)
    with GpuMatcher(0) as m:
        m.set_stream(None)
        n = 1_000_000
        for nul, tag in ((0, "NUL-free"), (1000, "0x00 at p=1e-3"), (-3, "0x00 in byte 3")):
            sp = K.SynthParams.make(seed=1234, needle=NEEDLE, plant_permille=100, nul_ppm=max(nul, 0))
            d_a, d_o, d_l, pb = device_arena(m, None, 1500, n, sp)
            if nul == -3:
                d_a[: n * 1504].view(n, 1504)[:, 3] = 0
                torch.cuda.synchronize()
            m.set_patterns([NEEDLE])
            m.attach_arena(d_a, d_o, d_l)
            leg(m, f"flat 1Mx1500B x1, {tag}", pb, args, nul == 0)
            m.set_patterns(tokens)
            m.attach_arena(d_a, d_o, d_l)
            leg(m, f"fused 1Mx1500B x97, {tag}", pb, args, nul == 0)
            del d_a, d_o, d_l
            torch.cuda.empty_cache()
        sp = K.SynthParams.make(seed=1234, needle=NEEDLE, plant_permille=100)
        d_a, d_o, d_l, pb = device_arena(m, zipf_lengths(n), 0, n, sp)
        m.set_patterns([NEEDLE])
        m.attach_arena(d_a, d_o, d_l)
        leg(m, "packed 1M Zipf 64-9000B x1, NUL-free", pb, args, True)
        del d_a, d_o, d_l
        torch.cuda.empty_cache()
        n64 = 12_000_000
        d_a, d_o, d_l, pb = device_arena(m, None, 64, n64, sp)
        m.set_patterns(tokens)
        m.attach_arena(d_a, d_o, d_l)
        leg(m, "fused 12Mx64B x97, NUL-free", pb, args, True)
        del d_a, d_o, d_l
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
