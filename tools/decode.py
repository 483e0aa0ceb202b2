"""What kmpgpu_load_decoded costs, kernel by kernel, against kmpgpu_load_selected with all bits set on the same arena (DESIGN.md §3.23;
profiles/decode.txt).

    python3 tools/decode.py [--reps 20] [--shapes 1500,64] [--out profiles/decode.txt]

Shapes: 1 M x 1500 B and 1 M x 64 B, lower-case letters.  Escape densities: none; one `%2e` per payload; every byte escaped (the payload
is `%41` x L / 3).  Per shape and density, alternating inside each round so that drift hits them alike:
  (a)  kmpgpu_load_decoded (no flags) under kmpgpu_profile_begin .. _end: the four recorded spans -- decoded lengths, the two scan
       kernels, index, write -- and kernel_ms of kmpgpu_last_timing (first decode kernel to the write's end);
  (b)  kmpgpu_load_selected with every bit set, the bitmap on the device: kernel_ms of kmpgpu_last_timing.  It moves the same bytes
       where nothing is escaped, minus the extra read of the arena that the lengths pass makes.
Medians with the quartiles of --reps repeats after a warm-up; (a) / (b) is the ratio DESIGN.md quotes."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import DECODE_PERCENT, GpuMatcher  # noqa: E402

N = 1_000_000
DENSITIES = ["none", "one %2e per payload", "every byte escaped"]
SPANS = ["lengths", "scan x 2", "index", "write"]


def med_q(v):
    if len(v) < 2:
        return (v[0], v[0], v[0]) if v else (float("nan"),) * 3
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def fmt(v):
    m, q1, q3 = med_q(v)
    return f"{m:.3f} [{q1:.3f}, {q3:.3f}]"


def make_arena(L, density):
    """N payloads of L bytes in slots of round_up(L, 16), padding 0x00, and the 64 bytes K.arena_layout leaves behind them, on the device"""
    slot = max(16, (L + 15) // 16 * 16)
    if density == "every byte escaped":
        one = torch.from_numpy(np.frombuffer((b"%41" * (L // 3 + 1))[:L] + b"\0" * (slot - L), dtype=np.uint8).copy()).cuda()
        return torch.cat([one.repeat(N), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    g = torch.Generator(device="cuda")
    g.manual_seed(L)
    a = torch.randint(97, 123, (N, slot), dtype=torch.uint8, device="cuda", generator=g)
    a[:, L:] = 0
    if density != "none":
        a[:, 5:8] = torch.tensor(list(b"%2e"), dtype=torch.uint8, device="cuda")
    return torch.cat([a.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1500,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode.txt"))
    args = ap.parse_args()
    src, dst, sel = GpuMatcher(0), GpuMatcher(0), GpuMatcher(0)
    g = dst._g
    lines = [f"kmpgpu_load_decoded against kmpgpu_load_selected (all bits), medians [q1, q3] of {args.reps} alternating repeats, ms "
             f"(GPU: {torch.cuda.get_device_name(0)})"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    try:
        for L in [int(s) for s in args.shapes.split(",") if s]:
            off, ln, nbytes = K.arena_layout(None, L, N)
            d_o = torch.from_numpy(off.astype(np.int64)).cuda()
            d_l = torch.from_numpy(ln.astype(np.int32)).cuda()
            ones = torch.full(((N + 63) // 64,), -1, dtype=torch.int64, device="cuda")
            say(f"shape {L}: {N} payloads of {L} bytes, {nbytes} slot bytes")
            for density in DENSITIES:
                d_a = make_arena(L, density)
                assert d_a.numel() == nbytes
                torch.cuda.synchronize()
                src.attach_arena(d_a, d_o, d_l)
                st = _lib.DecodeStats()
                n_out = C.c_uint64()

                def call_a():
                    dst.profile_begin(8)
                    rc = g.kmpgpu_load_decoded(dst._ctx, src._ctx, DECODE_PERCENT, 0, None, None, C.byref(st))
                    spans = dst.profile_end(8)
                    assert rc == 0 and st.n_payloads == N and len(spans) == len(SPANS)
                    return dst.last_timing().kernel_ms, spans

                def call_b():
                    assert g.kmpgpu_load_selected(sel._ctx, src._ctx, ones.data_ptr(), 1, C.byref(n_out)) == 0 and n_out.value == N
                    return sel.last_timing().kernel_ms

                for _ in range(3):
                    call_a(); call_b()
                ka, kb, per = [], [], [[] for _ in SPANS]
                for _ in range(args.reps):
                    k, spans = call_a()
                    ka.append(k)
                    for i, x in enumerate(spans):
                        per[i].append(float(x))
                    kb.append(call_b())
                ma, mb = med_q(ka)[0], med_q(kb)[0]
                moved = int(st.bytes_in) * 2 + int(st.bytes_out)
                say(f"  {density}: {int(st.n_changed)} payloads changed, {int(st.bytes_in)} -> {int(st.bytes_out)} bytes; (a) kernel_ms {fmt(ka)} "
                    f"({moved / ma / 1e6:.0f} GB/s over two reads and one write); " + ", ".join(f"{name} {fmt(v)}" for name, v in zip(SPANS, per))
                    + f"; (b) load_selected kernel_ms {fmt(kb)}; (a) / (b) {ma / mb:.2f}")
                src.attach_arena(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"),
                                 torch.zeros(0, dtype=torch.int32, device="cuda"))
                del d_a
                torch.cuda.empty_cache()
    finally:
        for m in (src, dst, sel):
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
