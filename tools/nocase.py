"""Case-insensitive patterns: the fold against a device-to-device copy of the same bytes, and first / repeat scans nocase against
case-sensitive ("Case-insensitive patterns"; profiles/nocase.txt).

    rocprofv3 --kernel-trace --stats -- python3 tools/nocase.py

Arena: the headline one, 1 M x 1500 B synthetic (S1, one 16-byte pattern), and the same arena with strings.txt's 97 tokens (fused
pass).  The fold runs inside the first nocase scan after an attach (kernel_ms); first - repeat is its cost as the scan sees it, the
kernel trace has kmp_fold_kernel on its own.  Repeat scans of the two kinds alternate, so that drift hits both alike."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

REPS = 30


def med(xs):
    return statistics.median(xs)


def main():
    n, L, stride = 1_000_000, 1500, 1504
    needle = b"NEEDLE_16B_PATRN"
    sp = K.SynthParams.make(seed=1234, needle=needle, plant_permille=100)
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_copy = torch.empty_like(d_arena)
    span = n * stride
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    with GpuMatcher(0) as m:
        m.set_stream(None)
        m.fixed_index(d_off, d_len, L, 16)
        m.synth_fill(d_arena, d_off, d_len, sp)
        m.sync()
        torch.cuda.synchronize()

        # the device-to-device copy of the span the fold reads and writes
        copy_ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d_copy[:span].copy_(d_arena[:span])
            e1.record()
            e1.synchronize()
            copy_ms.append(e0.elapsed_time(e1))
        c = med(copy_ms)
        print(f"span {span} B ({span / 1e9:.3f} GB); D2D copy (torch copy_) median {c:.3f} ms = {2 * span / c / 1e9:.2f} TB/s "
              f"(read + write), min {min(copy_ms):.3f} ms")

        for name, pats in (("headline: 1 x 16-byte pattern", [needle]), (f"strings.txt x {len(tokens)} (fused)", tokens)):
            first, rep_nc, rep_cs = [], [], []
            counts = {}
            for it in range(REPS):
                # nocase: attach (the fold goes stale), first scan = fold + scan, then a repeat
                m.set_patterns(pats, nocase=True)
                m.attach_arena(d_arena, d_off, d_len)
                got, t = m.scan()
                first.append(t.kernel_ms)
                got, t = m.scan()
                rep_nc.append(t.kernel_ms)
                counts["nocase"] = got
                launches_nc = t.launches
                m.set_patterns([p.lower() for p in pats])            # the folded set, case-sensitive
                got, t = m.scan()
                rep_cs.append(t.kernel_ms)
                counts["folded"] = got
                launches_cs = t.launches
            if len(pats) == 1:                                           # the planted needles, as written in upper case: nocase finds them all
                assert int(counts["nocase"][0]) == K.synth_count_planted(sp, n, L) and int(counts["folded"][0]) == 0
            f, r, s = med(first), med(rep_nc), med(rep_cs)
            print(f"{name}: launches nocase {launches_nc} / folded case-sensitive {launches_cs}; "
                  f"first nocase scan {f:.3f} ms, repeat nocase {r:.3f} ms, case-sensitive {s:.3f} ms "
                  f"(repeat / case-sensitive {r / s:.4f}); first - repeat (the fold) {f - r:.3f} ms = {(f - r) / c:.3f} x the copy "
                  f"[min first {min(first):.3f}, repeat {min(rep_nc):.3f}, cs {min(rep_cs):.3f}]")
    del d_arena, d_off, d_len, d_copy
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
