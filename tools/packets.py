"""kmpgpu_scan_packets against kmpgpu_scan and kmpgpu_scan_offsets with cap = 0 ("Which payloads match";
profiles/packets.txt).

    python3 tools/packets.py [--reps 30] [--out profiles/packets.txt]
    rocprofv3 --kernel-trace --stats -- python3 tools/packets.py --reps 3        (the reduce kernel on its own)

Shapes, all on 1 M x 1500 B payloads (the bench arena, synthetic S1):
  (a) the 16-byte needle, planted in ~10 % of the payloads (streaming kernel);
  (b) strings.txt's 97 tokens (fused pass);
  (c) one-letter text x a 16-byte pattern of that letter: every start offset matches (1.5e9 matches);
  (d) 1 000 random patterns of 4..12 bytes (fused, classed groups).
Times are medians of --reps calls after a warm-up, HIP events on the context's stream around each call: for the offsets
and packets calls that is everything they enqueue (zeroing, scan launches, reduces, the small downloads); kmpgpu_scan is
its own kernel_ms (scan + count reduce).  The three calls alternate, so that drift hits them alike."""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packets.txt"))
    args = ap.parse_args()
    n, L, stride = 1_000_000, 1500, 1504
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    rng = random.Random(1000)
    rand1000 = [bytes(rng.randrange(ord("a"), ord("z") + 1) for _ in range(rng.randrange(4, 13))) for _ in range(1000)]
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"kmpgpu_scan_packets vs kmpgpu_scan / kmpgpu_scan_offsets(cap = 0), {n} x {L} B, medians of {args.reps} "
             f"(GPU: {torch.cuda.get_device_name(0)})"]
    shapes = [("a", "needle, ~10 % of payloads", K.SynthParams.make(seed=1234, needle=needle, plant_permille=100), [needle]),
              ("b", "strings.txt x 97 (fused)", K.SynthParams.make(seed=1234, needle=needle, plant_permille=100), tokens),
              ("c", "one-letter text x 'a' * 16 (dense)", K.SynthParams.make(seed=1234, needle=b"a", plant_permille=0, lo=ord("a"), span=1),
               [b"a" * 16]),
              ("d", "1000 random 4..12-byte patterns", K.SynthParams.make(seed=1234, needle=needle, plant_permille=100), rand1000)]
    with GpuMatcher(0) as m:
        m.set_stream(stream.cuda_stream)
        m.fixed_index(d_off, d_len, L, 16)
        for key, name, sp, pats in shapes:
            m.synth_fill(d_arena, d_off, d_len, sp)
            m.sync()
            m.set_patterns(pats)
            m.attach_arena(d_arena, d_off, d_len)
            want, _ = m.scan()
            res = m.scan_packets()
            _, found, cnt = m.scan_offsets(0)
            assert res["counts"].tolist() == want.tolist() == cnt.tolist() and found == int(want.sum())
            assert int(res["any"].sum()) <= n and (res["pkt_counts"] <= res["counts"]).all()
            if key == "a":
                assert int(res["pkt_counts"][0]) == int(res["any"].sum()) == K.synth_count_planted(sp, n, L)
            if key == "c":
                assert int(res["pkt_counts"][0]) == n and int(want[0]) == n * (L - 15)
            sc, off, pk, pk_own, launches = [], [], [], [], 0
            for _ in range(3):                                       # warm-up
                m.scan(); m.scan_offsets(0); m.scan_packets()
            for _ in range(args.reps):
                sc.append(m.scan()[1].kernel_ms)
                off.append(timed(stream, lambda: m.scan_offsets(0))[0])
                ms, r = timed(stream, lambda: m.scan_packets())
                pk.append(ms)
                pk_own.append(r["timing"].kernel_ms)
                launches = r["timing"].launches
            s, o, p, q = (statistics.median(x) for x in (sc, off, pk, pk_own))
            lines.append(f"({key}) {name}: {len(pats)} patterns, {int(want.sum())} matches, {int(res['any'].sum())} payloads hit; "
                         f"scan {s:.3f} ms, offsets(cap 0) {o:.3f} ms, packets {p:.3f} ms (kernel_ms {q:.3f}, {launches} launches); "
                         f"packets / offsets {p / o:.3f}, packets / scan {p / s:.3f}")
            print(lines[-1], flush=True)
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
