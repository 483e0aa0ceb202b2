#!/usr/bin/env python3
"""What a linked row costs, on 1 M x 1500 B synthetic payloads, medians of --reps rounds:

    python3 tools/links.py [--parent-lib <libkmpgpu.so of the parent commit>] [--reps 10] [--out profiles/links.txt]

  gather    the gather alone: kmpgpu_link_rows' t.kernel_ms, taken by events of its own around the translation's kernels (the ranks of
            a bitmap and the gather; src's pass is not in it), per map kind at 1, 100 and 1 000 rows of src's 1 000 rules.  The bitmap
            and the index name every payload, so all three kinds move the same rows.
  link      kmpgpu_link_rows whole (wall clock, it is synchronous) against src's kmpgpu_scan_rules with every output NULL in the same
            rounds: the difference is the link.
  rule      one rule over three buffers -- three contexts over the same payloads, one pattern each -- through three links and
            kmpgpu_scan_rules, the verdict left on the device, against the host route like for like: every context's row downloaded
            (scan_packets with hits) and combined with numpy.
  parent    with --parent-lib: kmpgpu_scan_rules (5 patterns, 100 rules) and kmpgpu_load_fields(raw_uri) on a context without links,
            this build and the parent's by turns in the same rounds; the parent's own min .. max is printed, and whether this
            build's median lies inside it.
"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/gpu_support.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

NEEDLE = b"NEEDLE_16B_PATRN"
PATS = [NEEDLE, b"NEEDLE", b"16B_", b"PATRN", b"qzj"]


def matcher_on(path):
    """a GpuMatcher on another build of the library (one without the links included)"""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.GPU_API.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    return GpuMatcher(0, lib=lib)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def spread(v):
    return f"{statistics.median(v):.3f} (min {min(v):.3f} max {max(v):.3f})"


def null_scan_rules(m):
    _lib.gpu_check(m._g.kmpgpu_scan_rules(m._ctx, None, None, None, None, None), "kmpgpu_scan_rules")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links.txt"))
    args = ap.parse_args()
    n, L, reps = args.n, 1500, args.reps
    rng = random.Random(5)

    off, ln, nbytes = K.arena_layout(None, L, n)
    stride = int(off[1] - off[0]) if n > 1 else nbytes
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    lines = [f"tools/links.py: {n} x {L} B synthetic payloads, needle in ~10 %, medians of {reps} (GPU: {torch.cuda.get_device_name(0)}); "
             f"parent library: {'yes' if args.parent_lib else 'none given'}", ""]

    def ctx(pats, lib_path=None):
        m = matcher_on(lib_path) if lib_path else GpuMatcher(0)
        m.set_patterns(pats)
        m.attach_arena(d_arena, d_off, d_len)
        return m

    b = GpuMatcher(0)
    b.fixed_index(d_off, d_len, L, 16)
    b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=NEEDLE, plant_permille=100))
    torch.cuda.synchronize()
    b.close()

    # -- gather, link ---------------------------------------------------------------------------------------------------------------
    src, dst = ctx(PATS), ctx([b"unused"])
    src.set_rules([([rng.randrange(len(PATS))], []) if q % 2 else ([0], [rng.randrange(1, len(PATS))]) for q in range(1000)])
    dst.set_links(1000)
    every = np.ones(n, dtype=bool)
    ident = np.arange(n, dtype=np.uint32)
    maps = {"same": None, "bitmap": torch.from_numpy(K.matcher.select_words(every, n).view(np.int64)).cuda(),
            "index": torch.from_numpy(ident.view(np.int32)).cuda()}
    lines.append("gather: kmpgpu_link_rows t.kernel_ms (the translation's kernels alone), ms")
    for rows in (1, 100, 1000):
        for kind, mp in maps.items():
            v = [dst.link_rows(0, src, "rules", rows=range(rows), map=mp).kernel_ms for _ in range(reps + 1)][1:]
            lines.append(f"  {kind:6s} {rows:5d} rows   {spread(v)}   ({rows * n / 8 / 1e6:.1f} MB each way, {2 * rows * n / 8 / 1e9 / statistics.median(v):.2f} TB/s)")
    lines += ["", "link: kmpgpu_link_rows whole against src's kmpgpu_scan_rules (outputs NULL), wall clock, ms"]
    for rows in (1, 100, 1000):
        a, s = [], []
        for _ in range(reps + 1):
            s.append(wall(lambda: null_scan_rules(src))[0])
            a.append(wall(lambda: dst.link_rows(0, src, "rules", rows=range(rows)))[0])
        a, s = a[1:], s[1:]
        lines.append(f"  {rows:5d} rows of 1000   link_rows {spread(a)}   scan_rules {spread(s)}   difference {statistics.median(a) - statistics.median(s):.3f}")
    src.close()
    dst.close()

    # -- the three-buffer rule --------------------------------------------------------------------------------------------------------
    cap, b0, b1, b2 = ctx([b"unused"]), ctx([NEEDLE]), ctx([b"16B_"]), ctx([b"qzj"])
    cap.set_links(3)
    cap.set_rules([([cap.link(0), cap.link(1)], [cap.link(2)])])

    def by_links():
        for q, m in enumerate((b0, b1, b2)):
            cap.link_rows(q, m, "patterns")
        _lib.gpu_check(cap._g.kmpgpu_scan_rules(cap._ctx, None, None, None, None, None), "kmpgpu_scan_rules")

    def by_host():
        r = [m.scan_packets(hits=True)["hits"][0] for m in (b0, b1, b2)]
        return r[0] & r[1] & ~r[2]

    lk, ho = [], []
    for _ in range(reps + 1):
        lk.append(wall(by_links)[0])
        t, verdict = wall(by_host)
        ho.append(t)
    same = bool(np.array_equal(cap.scan_rules(hits=True)["hits"][0], verdict))
    lines += ["", "rule: one rule over three buffers, wall clock, ms",
              f"  three links + scan_rules, verdict on the device   {spread(lk[1:])}",
              f"  three scan_packets(hits) + numpy, verdict on the host   {spread(ho[1:])}",
              f"  verdicts equal: {same} ({int(verdict.sum())} payloads)"]
    for m in (cap, b0, b1, b2):
        m.close()

    # -- against the parent -----------------------------------------------------------------------------------------------------------
    if args.parent_lib:
        rules = [([rng.randrange(len(PATS))], [rng.randrange(len(PATS))]) for _ in range(100)]
        ms = {"parent": ctx(PATS, args.parent_lib), "this": ctx(PATS)}
        fd = {"parent": matcher_on(args.parent_lib), "this": GpuMatcher(0)}
        for k in ms:
            ms[k].set_rules(rules)
            fd[k].set_patterns([b"unused"])
        t_rules, t_fields = {k: [] for k in ms}, {k: [] for k in ms}
        for _ in range(reps + 1):
            for k in ("parent", "this"):
                t_rules[k].append(wall(lambda: null_scan_rules(ms[k]))[0])
                t_fields[k].append(wall(lambda: fd[k].load_fields(ms[k], "raw_uri"))[0])
        lines += ["", "parent: a context without links, this build and the parent's by turns, wall clock, ms"]
        for name, t in (("kmpgpu_scan_rules (5 patterns, 100 rules)", t_rules), ("kmpgpu_load_fields(raw_uri)", t_fields)):
            p, c = t["parent"][1:], t["this"][1:]
            inside = min(p) <= statistics.median(c) <= max(p)
            lines.append(f"  {name}: parent {spread(p)}   this build {spread(c)}   ratio {statistics.median(c) / statistics.median(p):.4f}   "
                         f"median inside the parent's min .. max: {'yes' if inside else 'NO'}")
        for m in list(ms.values()) + list(fd.values()):
            m.close()
    else:
        lines += ["", "parent: not measured (no --parent-lib)"]

    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
