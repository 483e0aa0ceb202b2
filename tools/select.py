"""What kmpgpu_load_selected costs, against its ceiling and against what a caller had to do before it (DESIGN.md §3.14;
profiles/select.txt).

    python3 tools/select.py [--reps 30] [--host-reps 5] [--shapes 1500,64,zipf] [--out profiles/select.txt]
    rocprofv3 --kernel-trace --stats -- python3 tools/select.py --reps 3 --host-reps 0 --no-cascade --out ''     (where the time of (a) goes)

Shapes: 1 M x 1500 B, 1 M x 64 B and the Zipf-length shape of bench.py --full (1 M payloads, 64..9000 B), synthetic text (kmp_synth.h).
Selection densities 0.1 %, 1 %, 10 %, 50 % and 100 %, a seeded random bitmap each.  Per shape and density, the variants alternating
inside each round so that drift hits them alike:
  (a)  kmpgpu_load_selected through the raw ABI with the bitmap words on the host: kernel_ms of kmpgpu_last_timing (first selection
       kernel to the copy's end) and the wall time of the call (upload of the bitmap, the host's wait for the totals, the index pass and
       the side tables of the new arena included);
  (b)  the ceiling: one device-to-device hipMemcpyAsync of as many bytes as the selected slots hold (torch copy_ of a contiguous byte
       tensor), between HIP events;
  (c)  what a caller does without the call: kmpgpu_arena_download of the whole arena, the selection with numpy on the host,
       kmpgpu_load_arena of the subset; wall time, --host-reps repeats (a second or more each).
Medians with the quartiles of --reps repeats after a warm-up.
  (d)  the cascade on the 1500-byte shape, the benchmark's needle planted in ~10 % of the payloads: stage 1 kmpgpu_scan_packets of the
       needle, kmpgpu_load_selected of its any[], stage 2 the 1 000 patterns of tools/manypat.py over the subset -- against the same
       1 000 patterns over the whole arena.  The per-pattern payload counts of stage 2 are compared exactly with the full pass's hit
       rows restricted on the host to the selected payloads."""
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
from multithreading_string_matching_amd.matcher import OPT_FUSED, GpuMatcher, select_words  # noqa: E402

NEEDLE = b"NEEDLE_16B_PATRN"
DENSITIES = [0.001, 0.01, 0.1, 0.5, 1.0]


def slot_bytes(ln):
    ln = ln.astype(np.int64)
    return np.maximum(16, (ln + 15) // 16 * 16)


def med_q(v):
    if len(v) < 2:
        return (v[0], v[0], v[0]) if v else (float("nan"),) * 3
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def fmt(v):
    m, q1, q3 = med_q(v)
    return f"{m:.3f} [{q1:.3f}, {q3:.3f}]"


def make_shape(m, name):
    n = 1_000_000
    sp = K.SynthParams.make(seed=1234, needle=NEEDLE, plant_permille=100)
    if name == "zipf":
        rng = np.random.default_rng(4)
        ranks = np.arange(1, 9000 - 64 + 2)
        pz = 1.0 / ranks ** 1.1
        pz /= pz.sum()
        lens = (64 + rng.choice(len(ranks), size=n, p=pz)).astype(np.uint32)
        off, ln, nbytes = K.arena_layout(lens, 0, n)
    else:
        off, ln, nbytes = K.arena_layout(None, int(name), n)
    d_a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_o = torch.from_numpy(off.astype(np.int64)).cuda()
    d_l = torch.from_numpy(ln.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    m.synth_fill(d_a, d_o, d_l, sp)
    m.sync()
    return d_a, d_o, d_l, off.astype(np.int64), ln


def host_select(m_src, m_tmp, sel):
    """(c): the whole arena to the host, the subset picked with numpy, uploaded again"""
    arena, off, ln = m_src.arena_download()
    idx = np.flatnonzero(sel)
    sl = ln[idx]
    slot = slot_bytes(sl)
    new_off = np.zeros(len(idx), dtype=np.uint64)
    if len(idx) > 1:
        new_off[1:] = np.cumsum(slot[:-1]).astype(np.uint64)
    total = int(slot.sum())
    if len(idx) and (ln == ln[0]).all():
        st = int(slot_bytes(ln[:1])[0])
        sub = arena[:len(ln) * st].reshape(len(ln), st)[idx].reshape(-1)
    else:
        take = np.zeros(len(arena), dtype=bool)
        mark = np.zeros(len(arena) + 1, dtype=np.int8)                 # +1 at a selected slot's start, -1 at its end
        np.add.at(mark, off[idx].astype(np.int64), 1)
        np.add.at(mark, off[idx].astype(np.int64) + slot, -1)
        take[:] = np.cumsum(mark[:-1], dtype=np.int8) > 0
        sub = arena[take]
    assert len(sub) == total
    m_tmp.load_arena(np.concatenate([sub, np.zeros(64, np.uint8)]), new_off, sl)
    return len(idx)


def popcount_rows(words):
    table = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)
    return table[words.view(np.uint8)].reshape(words.shape[0], -1).sum(axis=1, dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--shapes", default="1500,64,zipf")
    ap.add_argument("--no-cascade", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select.txt"))
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    src, dst, tmp = GpuMatcher(0), GpuMatcher(0), GpuMatcher(0)
    for m in (src, dst, tmp):
        m.set_stream(stream.cuda_stream)
        m.set_patterns([NEEDLE])
    g = dst._g
    lines = [f"kmpgpu_load_selected, medians [q1, q3] of {args.reps} alternating repeats ((c): {args.host_reps}), ms (GPU: {torch.cuda.get_device_name(0)})"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    try:
        for shape in [s for s in args.shapes.split(",") if s]:
            d_a, d_o, d_l, off, ln = make_shape(src, shape)
            n = len(ln)
            src.attach_arena(d_a, d_o, d_l)
            slots = slot_bytes(ln)
            scratch = torch.empty(int(slots.sum()) + 64, dtype=torch.uint8, device="cuda")
            say(f"shape {shape}: {n} payloads, {int(ln.astype(np.int64).sum())} payload bytes, {int(slots.sum())} slot bytes")
            for p in DENSITIES:
                rng = np.random.default_rng(int(p * 1000))
                sel = np.ones(n, bool) if p >= 1.0 else rng.random(n) < p
                words = select_words(sel, n)
                nbytes = int(slots[sel].sum())
                n_out = C.c_uint64()

                def call_a():
                    t0 = time.perf_counter()
                    rc = g.kmpgpu_load_selected(dst._ctx, src._ctx, words.ctypes.data, 0, C.byref(n_out))
                    wall = (time.perf_counter() - t0) * 1e3
                    assert rc == 0 and n_out.value == int(sel.sum())
                    return dst.last_timing().kernel_ms, wall

                def call_b():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record(stream)
                        scratch[:nbytes].copy_(d_a[:nbytes], non_blocking=True)
                        e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                for _ in range(3):
                    call_a(); call_b()
                ka, wa, tb = [], [], []
                for _ in range(args.reps):
                    k, w = call_a()
                    ka.append(k); wa.append(w); tb.append(call_b())
                tc = []
                for r in range(args.host_reps + (1 if args.host_reps else 0)):
                    t0 = time.perf_counter()
                    got = host_select(src, tmp, sel)
                    if r:
                        tc.append((time.perf_counter() - t0) * 1e3)
                    assert got == int(sel.sum())
                if args.host_reps:
                    assert tmp.scan()[0].tolist() == dst.scan()[0].tolist()          # (c) and (a) built the same subset
                    tmp.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
                ma, mb = med_q(ka)[0], med_q(tb)[0]
                say(f"  density {p * 100:5.1f} %: {int(sel.sum())} payloads, {nbytes} slot bytes; (a) kernel_ms {fmt(ka)} ({2 * nbytes / ma / 1e6:.0f} GB/s read + written), "
                    f"call wall {fmt(wa)}; (b) memcpy {fmt(tb)} ({2 * nbytes / mb / 1e6:.0f} GB/s); (b) / (a) {mb / ma:.3f}; "
                    f"(c) host round trip wall {fmt(tc) if tc else 'not measured'}")
            if shape == "1500" and not args.no_cascade:
                cascade(src, dst, tmp, stream, n, say, args.reps)
            src.attach_arena(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"),
                             torch.zeros(0, dtype=torch.int32, device="cuda"))
            dst.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
            del d_a, d_o, d_l, scratch
            torch.cuda.empty_cache()
    finally:
        for m in (src, dst, tmp):
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def cascade(src, dst, full, stream, n, say, reps):
    """(d): src holds the 1500-byte arena (borrowed) under the needle; `full` gets the same arena under the 1 000 patterns"""
    rng = random.Random(7)
    pats = None
    for npat in (100, 256, 257, 1000):                               # tools/manypat.py draws its sets in this order from this seed
        pats = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(4, 13))) for _ in range(npat)]
    W = (n + 63) // 64
    g = src._g
    full.set_option(OPT_FUSED, 1); dst.set_option(OPT_FUSED, 1)
    full.set_patterns(pats); dst.set_patterns(pats)
    full.attach_arena(*src._keep)
    any1 = np.zeros(W, dtype=np.uint64)
    n_out = C.c_uint64()

    def run_cascade():
        assert g.kmpgpu_scan_packets(src._ctx, None, any1.ctypes.data, None, None, None) == 0
        assert g.kmpgpu_load_selected(dst._ctx, src._ctx, any1.ctypes.data, 0, C.byref(n_out)) == 0
        return dst.scan_packets()

    def run_full():
        return full.scan_packets()

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    # exactness: stage 2's payload counts == the full pass's rows restricted to the selected payloads
    res = run_cascade()
    rows = np.zeros((len(pats), W), dtype=np.uint64)
    assert g.kmpgpu_scan_packets(full._ctx, None, None, rows.ctypes.data, None, None) == 0
    want = popcount_rows(rows & any1[None, :])
    assert res["pkt_counts"].tolist() == want.tolist(), "cascade: stage 2 differs from the restricted full pass"
    del rows
    for _ in range(2):
        run_cascade(); run_full()
    tc, tf, t2 = [], [], []
    for _ in range(reps):
        w, r = wall(run_cascade)
        tc.append(w); t2.append(r["timing"].kernel_ms)
        tf.append(wall(run_full)[0])
    say(f"  (d) cascade, needle -> 1 000 patterns: {int(n_out.value)} of {n} payloads selected; stage 1 + selection + stage 2 wall {fmt(tc)} "
        f"(stage 2 kernel_ms {fmt(t2)}); the 1 000 patterns over the whole arena wall {fmt(tf)}; full / cascade {med_q(tf)[0] / med_q(tc)[0]:.2f}; "
        f"payload counts == restricted full pass: yes ({int(want.sum())} (pattern, payload) pairs)")
    full.set_option(OPT_FUSED, 2); dst.set_option(OPT_FUSED, 2)
    full.set_patterns([NEEDLE]); dst.set_patterns([NEEDLE])
    full.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


if __name__ == "__main__":
    main()
