"""What the regex rows (kmpgpu_set_regexes) cost (profiles/regex.txt).

    python3 tools/regex.py --parent-lib <libkmpgpu.so of the parent commit> [--reps 30] [--out profiles/regex.txt]

All on 1 M x 1500 B payloads (the bench arena, synthetic S1: text of a..z, the bench needle planted in every tenth payload), contexts on one
device arena, HIP events on the contexts' stream around each call, the contexts alternating inside every round so that drift hits them
alike; medians of --reps rounds after a warm-up, with the smallest, the quartiles and the largest.
  (1) unchanged path    kmpgpu_scan_rules, strings.txt's 97 tokens and 100 generated rules: (a) the parent commit's library (--parent-lib;
                        left out without it) against (b) this tree's with no expressions set.  The outputs must be equal.  What is
                        claimed is "within the run-to-run spread of the parent": both spreads are printed.
  (2) the kernel        kmpgpu_scan_regexes and the kernel alone from kmpgpu_profile_begin (the last launch) for 1, KMP_RX_TILE and 100
                        generated expressions, under the strlen rule and under whole payloads; then single expressions: literals only,
                        a run of 20 optional positions, and one behind a gate (the bench needle) that every tenth and that every
                        payload holds.  Beside each the share of the payloads it hits (a lane stops walking once every expression of
                        its tile without $ has accepted) and the time per (expression, text byte) as if every byte were walked.  The rows
                        of the first 4 096 payloads are checked against Python's re.
  (3) the grouped kernel  the same for expressions under KMPGPU_RX_GROUPS (kmp_regex_groups.hip), in the same run: one
                        flagged expression without a rule (the one of (2) that walks every byte, so the two kernels' figures stand side
                        by side), /(GET|POST|HEAD|PUT) \\//, one at KMPGPU_RX_MAX_EDGES rules, a full tile of KMP_RXG_TILE, 100 flagged
                        ones, and a mixed set, where the linear and the grouped launch are reported apart."""
import argparse
import ctypes as C
import os
import random
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import OPT_WHOLE_PAYLOAD, GpuMatcher  # noqa: E402

CHECKED = 4096                    # payloads whose rows are held to Python's re


def matcher_on(path):
    """a GpuMatcher on another build of the library (one without kmpgpu_set_regexes included)"""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.GPU_API.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    return GpuMatcher(0, lib=lib)


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def spread(v):
    q = statistics.quantiles(v, n=4)
    return f"{statistics.median(v):.3f} (min {min(v):.3f} q1 {q[0]:.3f} q3 {q[2]:.3f} max {max(v):.3f})"


def gen_rules(rng, n_rules, n_pat):
    """as tools/rules.py"""
    rules = []
    for _ in range(n_rules):
        pos, neg = [], []
        for _ in range(rng.randrange(1, 5)):
            (neg if rng.random() < 0.25 else pos).append(rng.randrange(n_pat))
        rules.append((pos, neg))
    return rules


def gen_exprs(n, seed=7):
    """expressions over text of a..z: three to five elements, classes of a few letters, every quantifier form"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        e = b""
        for _ in range(rng.randrange(3, 6)):
            lo = rng.randrange(0x61, 0x78)
            e += rng.choice([bytes([lo]), b"[%c-%c]" % (lo, lo + rng.randrange(1, 4)), b"[^%c-%c]" % (lo, 0x7A), b"\\w", b"."])
            e += rng.choice([b"", b"", b"?", b"+", b"*", b"{2}", b"{1,3}", b"{2,}"])
        out.append(e)
    return out


def gen_grouped(n, seed=11):
    """flagged expressions over text of a..z: a group of two or three alternatives of two or three elements each (no optional element
    at an alternative's end: a few edge rules, far from KMPGPU_RX_MAX_EDGES), sometimes optional or repeated, and a generated tail"""
    rng = random.Random(seed)

    def alt():
        e = b""
        for _ in range(rng.randrange(2, 4)):
            lo = rng.randrange(0x61, 0x78)
            e += rng.choice([bytes([lo]), b"[%c-%c]" % (lo, lo + rng.randrange(1, 4)), b"\\w", b"."]) + rng.choice([b"", b"", b"+", b"{2}"])
        return e

    tails = gen_exprs(n, seed)
    return [(b"(" + b"|".join(alt() for _ in range(rng.randrange(2, 4))) + b")" + rng.choice([b"", b"", b"?", b"+"]) + tails[i], {"groups": True})
            for i in range(n)]


def check_rows(m, exprs, head, gate_head, n):
    """the rows of the first CHECKED payloads of three expressions against Python's re; returns the mean share of payloads per expression"""
    W = (n + 63) // 64
    pc, hit_w = np.zeros(len(exprs), dtype=np.uint64), np.zeros((len(exprs), W), dtype=np.uint64)
    _lib.gpu_check(m._g.kmpgpu_scan_regexes(m._ctx, pc.ctypes.data, None, hit_w.ctypes.data, None, None), "kmpgpu_scan_regexes")
    for q in sorted({0, len(exprs) // 2, len(exprs) - 1}):
        expr, opt = (exprs[q], {}) if isinstance(exprs[q], bytes) else exprs[q]
        c = re.compile(expr[:-1] + b"\\Z" if expr.endswith(b"$") else expr)
        want = np.array([c.search(t) is not None for t in head]) & (gate_head if "gate" in opt else True)
        got = np.unpackbits(hit_w[q, :CHECKED // 64].view(np.uint8), bitorder="little").astype(bool)
        assert np.array_equal(got, want), f"the regex kernel and Python's re disagree on {expr!r}"
    return float(pc.sum()) / len(exprs) / n


def kernel_alone(c, stream, reps):
    tt, kk = [], []
    for rnd in range(3 + reps):
        c.profile_begin(64)
        dt, _ = timed(stream, lambda: c.scan_regexes())
        prof = c.profile_end(64)
        if rnd >= 3:
            tt.append(dt); kk.append(float(prof[-1]))
    return tt, kk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regex.txt"))
    args = ap.parse_args()
    n, L, stride = args.payloads, 1500, 1504
    assert n >= CHECKED
    needle = b"NEEDLE_16B_PATRN"
    tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    lines = [f"regex rows (kmpgpu_set_regexes), {n} x {L} B, KMP_RX_TILE {_lib.RX_TILE}, medians of {args.reps} alternating rounds with min / "
             f"quartiles / max, ms (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def head_of_arena():
        head = d_arena[:CHECKED * stride].cpu().numpy().reshape(CHECKED, stride)[:, :L]
        texts = [row.tobytes() for row in head]
        return texts, np.array([needle in t for t in texts])

    ms = {"b": GpuMatcher(0), "c": GpuMatcher(0)}
    if args.parent_lib:
        ms = {"a": matcher_on(args.parent_lib), **ms}
    try:
        for m in ms.values():
            m.set_stream(stream.cuda_stream)
        b, c = ms["b"], ms["c"]
        b.fixed_index(d_off, d_len, L, 16)
        b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=needle, plant_permille=100))
        b.sync()
        n_pat = len(tokens)
        rules = gen_rules(random.Random(100), 100, n_pat)
        for key, m in ms.items():
            m.set_patterns([needle] if key == "c" else tokens)
            m.attach_arena(d_arena, d_off, d_len)
        # ---- (1) the unchanged path
        for key in ("a", "b"):
            if key in ms:
                ms[key].set_rules(rules)
        res = {key: ms[key].scan_rules(hits=True) for key in ("a", "b") if key in ms}
        if "a" in res:
            for k in ("hits", "rule_pkt_counts", "any", "counts"):
                assert np.array_equal(res["a"][k], res["b"][k]), k
            assert res["a"]["timing"].launches == res["b"]["timing"].launches
        t = {key: [] for key in res}
        own = {key: [] for key in res}
        for rnd in range(3 + args.reps):                                 # three rounds of warm-up
            for key in res:
                dt, r = timed(stream, lambda: ms[key].scan_rules())
                if rnd >= 3:
                    t[key].append(dt); own[key].append(r["timing"].kernel_ms)
        line = f"(1) kmpgpu_scan_rules, {n_pat} tokens, {len(rules)} rules, no expressions set: "
        if "a" in t:
            line += f"(a) parent {spread(t['a'])}, kernel_ms {statistics.median(own['a']):.3f}; "
        line += f"(b) this tree {spread(t['b'])}, kernel_ms {statistics.median(own['b']):.3f}"
        if "a" in t:
            mb = statistics.median(t["b"])
            line += f"; (b) / (a) {mb / statistics.median(t['a']):.4f}; (b)'s median inside (a)'s range: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}"
        say(line)
        del res
        # ---- (2) the kernel
        head, gate_head = head_of_arena()

        def measure(label, exprs, part="(2)"):
            c.set_regexes(exprs)
            share = check_rows(c, exprs, head, gate_head, n)
            tt, kk = kernel_alone(c, stream, args.reps)
            k_med = statistics.median(kk)
            say(f"{part} {label}: {share * 100:.1f} % of the payloads per expression; kmpgpu_scan_regexes {spread(tt)}; regex kernel alone {spread(kk)}; "
                f"{k_med * 1e9 / len(exprs) / n / L:.3f} ps per (expression, text byte) of {len(exprs)} x {n} x {L}")

        for whole in (0, 1):
            c.set_option(OPT_WHOLE_PAYLOAD, whole)
            for n_rx in (1, _lib.RX_TILE, 100):
                measure(f"{'whole payloads' if whole else 'strlen rule'}, {n_rx} generated expression{'s' if n_rx > 1 else ''}", gen_exprs(n_rx))
        c.set_option(OPT_WHOLE_PAYLOAD, 0)
        measure("one expression of literals only, /qzjxkv/", [b"qzjxkv"])
        measure("one expression with a run of 20 optional positions, /q[a-m]{0,20}zz/", [b"q[a-m]{0,20}zz"])
        gated = [(b"qz[a-m]{2,}x$", {"gate": 0})]
        measure("one expression that walks every byte, /qz[a-m]{2,}x$/, ungated", [gated[0][0]])
        measure("the same behind a gate that every tenth payload holds", gated)
        # ---- (3) the grouped kernel: with every expression flagged it is the only regex launch, the last one of the profile
        flag = {"groups": True}
        measure("grouped kernel, one flagged expression without a rule, /qz[a-m]{2,}x$/ (the linear kernel's figure: four lines up)", [(gated[0][0], flag)], "(3)")
        measure("grouped kernel, /(GET|POST|HEAD|PUT) \\// (1 rule)", [(b"(GET|POST|HEAD|PUT) /", flag)], "(3)")
        measure(f"grouped kernel, /(ab|cd){{2,4}}e(f|gh)/ ({_lib.RX_MAX_EDGES} rules)", [(b"(ab|cd){2,4}e(f|gh)", flag)], "(3)")
        measure(f"grouped kernel, a full tile of {_lib.RXG_TILE} generated flagged expressions", gen_grouped(_lib.RXG_TILE), "(3)")
        measure("grouped kernel, 100 generated flagged expressions", gen_grouped(100), "(3)")
        # a mixed set: the linear launch, then the grouped one
        n_lin, n_grp = _lib.RX_TILE, _lib.RXG_TILE
        mixed = gen_exprs(n_lin) + gen_grouped(n_grp)
        c.set_regexes(mixed)
        check_rows(c, mixed, head, gate_head, n)
        lin_k, grp_k = [], []
        for rnd in range(3 + args.reps):
            c.profile_begin(64)
            c.scan_regexes()
            prof = c.profile_end(64)
            if rnd >= 3:
                lin_k.append(float(prof[-2])); grp_k.append(float(prof[-1]))
        say(f"(3) mixed set, {n_lin} unflagged + {n_grp} flagged: linear kernel {spread(lin_k)}, "
            f"{statistics.median(lin_k) * 1e9 / n_lin / n / L:.3f} ps per (expression, text byte); grouped kernel {spread(grp_k)}, "
            f"{statistics.median(grp_k) * 1e9 / n_grp / n / L:.3f} ps per (expression, text byte)")
        b.synth_fill(d_arena, d_off, d_len, K.SynthParams.make(seed=1234, needle=needle, plant_permille=1000))
        b.sync()
        c.attach_arena(d_arena, d_off, d_len)
        head, gate_head = head_of_arena()
        measure("the same behind a gate that every payload holds", gated)
    finally:
        for m in ms.values():
            m.close()
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
