"""GPU parity past the size thresholds of the dispatch in csrc/kmpgpu.hip: more than 65 535 patterns (launches split by
gridDim.y, 16-bit pattern index of the classed records), the sliced count reduce with and without KMPGPU_OPT_ACCUMULATE
(grids of more than 16 384 blocks), and the fused pass's work-unit pool when its first group is the wide kernel.
Every count is held to the CPU oracle (exact integer KMP).

Run on a real MI355X:  python -m pytest tests -m gpu
"""
import math
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import gm, reset  # noqa: E402,F401  (torch first)

import torch  # noqa: E402

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_FLAT, KERNEL_GENERAL, KERNEL_PACKED, MODE_AUTOMATON, MODE_FILTER, OPT_ACCUMULATE, OPT_BLOCKS_PER_CU, OPT_FUSED,
    OPT_FUSED_UNIT, OPT_KERNEL, OPT_MODE)

KERNEL_FUSED = 100          # test-only alias: auto kernel selection + the fused multi-pattern pass
# (mode, kernel) as in test_gpu_parity.VARIANTS
VARIANTS = ((MODE_FILTER, KERNEL_AUTO), (MODE_FILTER, KERNEL_FLAT), (MODE_FILTER, KERNEL_PACKED), (MODE_FILTER, KERNEL_FUSED), (MODE_FILTER, KERNEL_GENERAL),
            (MODE_AUTOMATON, KERNEL_GENERAL))
IDX16 = 0xFFFF              # the largest pattern index a launch (gridDim.y) or a classed record (16 bits) holds


def _select(gm, mode, kernel):
    gm.set_option(OPT_MODE, mode)
    gm.set_option(OPT_KERNEL, KERNEL_AUTO if kernel == KERNEL_FUSED else kernel)
    gm.set_option(OPT_FUSED, 1 if kernel == KERNEL_FUSED else 2 if kernel == KERNEL_AUTO else 0)


def _check_records(recs, arena, patterns, want, sample=400):
    """Offset records: as many per pattern as the oracle counts (ids past 65 535 included), and a sample of them really is
    the pattern's bytes, inside its payload and before the payload's first 0x00."""
    assert np.bincount(recs["pattern"].astype(np.int64), minlength=len(patterns)).tolist() == want.tolist()
    for r in recs[:: max(1, len(recs) // sample)]:
        k, s0, p = int(r["packet"]), int(r["offset"]), patterns[int(r["pattern"])]
        text = arena.payload(k)
        E = text.index(0) if 0 in text else len(text)
        assert text[s0:s0 + len(p)] == p and s0 + len(p) <= E, (k, s0, int(r["pattern"]))


# ------------------------------------------------------------------------------------------------
# A. more than 65 535 patterns
# ------------------------------------------------------------------------------------------------
def _text_payloads(rng, n, max_len, alphabet, extra=b"", nul_rate=0.1):
    out = []
    for _ in range(n):
        L = rng.randrange(0, max_len + 1)
        b = bytearray(rng.choice(alphabet) for _ in range(L))
        for _ in range(L // 60):
            if extra:
                b[rng.randrange(L)] = rng.choice(extra)
        if L and rng.random() < nul_rate:
            b[rng.randrange(L)] = 0
        out.append(bytes(b))
    return out


def _many_patterns(rng, payloads, n_total=70_000):
    """~70 000 patterns over "abcd", most of them distinct, with the cases of kmpgpu_set_patterns that turn on the pattern
    index placed right behind index 0xFFFF.  Returns (patterns, index of every placed case)."""
    seen = set()
    by_len = {}
    pool = [p[:p.index(0)] if 0 in p else p for p in payloads]
    pool = [p for p in pool if len(p) >= 40]

    def fresh(m, from_text):
        while True:
            if from_text:
                t = rng.choice(pool)
                s0 = rng.randrange(0, len(t) - m + 1)
                p = t[s0:s0 + m]
            else:
                p = bytes(rng.choice(b"abcd") for _ in range(m))
            if p not in seen:
                seen.add(p)
                by_len[m] = by_len.get(m, 0) + 1
                return p

    pats = []
    # all sixteen 2-byte patterns but one (it comes behind 0xFFFF), all 64 of 3 bytes
    twos = [bytes([x, y]) for x in b"abcd" for y in b"abcd"]
    seen.update(twos + [bytes([x, y, z]) for x in b"abcd" for y in b"abcd" for z in b"abcd"])
    pats += twos[:-1] + [bytes([x, y, z]) for x in b"abcd" for y in b"abcd" for z in b"abcd"]
    pats += [fresh(4, False) for _ in range(150)] + [fresh(5, False) for _ in range(300)] + [fresh(8, True) for _ in range(1000)]
    early_long = [fresh(rng.randrange(9, 41), True) for _ in range(2000)]
    pats += early_long
    while len(pats) < IDX16 - 3:
        pats.append(fresh(rng.randrange(6, 41), rng.random() < 0.5))
    placed = {}

    def put(name, p):
        placed[name] = len(pats)
        pats.append(p)

    put("long_fused", fresh(23, True))                  # 0xFFFC: a 9+-byte pattern still inside the 16-bit index: fused
    put("one_a", b"a")                                  # 0xFFFD: the first 1-byte pattern (rides along with the fused pass)
    put("four_last16", fresh(4, False))                 # 0xFFFE
    put("eight_last16", fresh(8, True))                 # 0xFFFF: the last index a classed record holds
    put("long_rest", fresh(17, True))                   # 0x10000: first occurrence past 0xFFFF, 9+ bytes: a streaming pass of its own
    put("four", fresh(4, False))                        # 4, 5 and 8 bytes past 0xFFFF: classed groups with the index field truncated
    put("five", fresh(5, False))
    put("eight", fresh(8, True))
    put("dup_long", early_long[7])                      # a duplicate of an early 9+-byte pattern: stays fused through first_pat
    for ch in b"bcdef":                                 # 1-byte patterns 2-6: three more ride along, 'e' and 'f' keep passes
        put("one_" + chr(ch), bytes([ch]))
    put("two", twos[-1])                                # a 2-byte pattern past 0xFFFF
    put("dup_one", b"a")
    put("dup_long_rest", pats[placed["long_rest"]])     # a duplicate of a rest pattern
    while len(pats) < n_total:
        r = rng.random()
        if r < 0.4:
            pats.append(fresh(rng.randrange(9, 41), True))
        elif r < 0.55:                                  # (of the 256 and 1024 there are: 240 and 900 at most)
            m = 4 if rng.random() < 0.1 and by_len.get(4, 0) < 240 else 5 if by_len.get(5, 0) < 900 else 8
            pats.append(fresh(m, m == 8))
        elif r < 0.75:
            pats.append(fresh(8, True))
        elif r < 0.85:
            pats.append(rng.choice(early_long))
        else:
            pats.append(rng.choice(pats[:IDX16]))
    return pats, placed


def test_many_patterns_past_the_16_bit_index(gm, oracle, tmp_path):
    """70 000 patterns: the streaming passes go in launches of at most 65 535 pattern ids (gridDim.y), the second one with
    its partial rows behind the first's; past index 0xFFFF, a new pattern of nine bytes or more leaves the fused pass (a
    classed record names the pattern that holds its tail in 16 bits), one of 4-8 bytes stays in a classed group with that
    field truncated (never read for it), a duplicate of an early long pattern stays fused; offset records carry 32-bit ids."""
    rng = random.Random(65536)
    payloads = _text_payloads(rng, 200, 300, b"abcd", extra=b"ef")
    pats, placed = _many_patterns(rng, payloads)
    n = len(pats)
    assert n > 65536 and max(placed.values()) > IDX16
    n_long = sum(len(p) >= 4 for p in pats)
    n_short = n - n_long
    assert n_long > 65535
    arena = K.HostArena.from_payloads(payloads)
    want, _ = oracle.count(arena.bytes, arena.off, arena.len, pats, threads=8)
    assert want.sum() > 100_000
    for name in ("long_fused", "long_rest", "four", "five", "eight", "eight_last16", "dup_long", "one_a", "one_e", "one_f", "two", "dup_long_rest"):
        assert want[placed[name]] > 0, name                 # every placed case is counted, so a dropped or misrouted one shows
    assert want[IDX16 + 1:].sum() > 1000
    uni_payloads = [p[:160].ljust(160, b"c") for p in payloads]
    uni = K.HostArena.from_payloads(uni_payloads)
    want_uni, _ = oracle.count(uni.bytes, uni.off, uni.len, pats, threads=8)
    try:
        gm.set_patterns(pats)
        for mode, kernel in VARIANTS:
            a, w = (uni, want_uni) if kernel == KERNEL_FLAT else (arena, want)
            _select(gm, mode, kernel)
            gm.load_arena(a)
            got, t = gm.scan()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, (mode, kernel, [(int(i), pats[int(i)], int(got[i]), int(w[i])) for i in bad[:5]])
            if kernel not in (KERNEL_AUTO, KERNEL_FUSED):
                # one launch per 65 535 pattern ids: the loop over them ran past its first iteration
                assert t.launches == math.ceil(n_long / 65535) + math.ceil(n_short / 65535), (mode, kernel, t.launches)
        gm.load_arena(arena)
        for fused in (1, 0):
            _select(gm, MODE_FILTER, KERNEL_FUSED if fused else KERNEL_PACKED)
            recs, found, counts = gm.scan_offsets(int(want.sum()) + 10)
            assert found == int(want.sum()) == len(recs) and counts.tolist() == want.tolist(), fused
            assert int(recs["pattern"].max()) > IDX16
            _check_records(recs, arena, pats, want)
    finally:
        reset(gm)

    # the command lines, with a pattern file of more than 65 536 tokens mostly cut out of the capture's payloads
    cap = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    runs = []
    for k in range(cap.n_pkts):
        text = cap.payload(k)
        run = bytearray()
        for ch in text + b"\0":
            if 33 <= ch < 127:
                run.append(ch)
            else:
                if len(run) >= 2:
                    runs.append(bytes(run))
                run = bytearray()
    tokens = []
    while len(tokens) < 70_000:
        if rng.random() < 0.8:
            t = rng.choice(runs)
            m = rng.randrange(1, min(len(t), 40) + 1)
            s0 = rng.randrange(0, len(t) - m + 1)
            tokens.append(t[s0:s0 + m])
        else:
            tokens.append(bytes(rng.randrange(33, 127) for _ in range(rng.randrange(1, 12))))
    pfile = tmp_path / "many_tokens.txt"
    pfile.write_bytes(b"\n".join(tokens) + b"\n")
    assert K.load_patterns(str(pfile)) == tokens
    want_cli, _ = oracle.count(cap.bytes, cap.off, cap.len, tokens, threads=8)
    assert int(np.count_nonzero(want_cli[IDX16 + 1:])) > 100
    expected = K.format_report(tokens, want_cli)
    for prog, extra in (("serial", []), ("openmp_data", ["3"])):
        r = subprocess.run([os.path.join(_lib.BINDIR, prog), os.path.join(DATA, "udp_1000.pcap"), str(pfile), *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (prog, r.stderr)
        lines = r.stdout.splitlines(keepends=True)
        assert lines and lines[-1].startswith("Elapsed time = ") and lines[-1].endswith(" seconds\n")
        assert "".join(lines[:-1]) == expected, prog


# ------------------------------------------------------------------------------------------------
# B. the sliced count reduce
# ------------------------------------------------------------------------------------------------
B_PATTERNS = [b"ab", b"abcab", b"z", b"abcabcabcab", b"ca", b"ab"]     # short, long, a 1-byte rider, 9+ bytes, short, a duplicate


def _small_payload_batch(seed, n, uniform_len=None):
    """An arena (bytes, offsets, lengths) of n payloads of 16-200 bytes (or all of uniform_len) over "abcdef" with a few 'z',
    planted 11-byte matches and some 0x00."""
    rng = np.random.default_rng(seed)
    lens = np.full(n, uniform_len, dtype=np.int64) if uniform_len else rng.integers(16, 201, n)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    probs = np.array([0.19] * 5 + [0.04, 0.01])
    text = rng.choice(np.frombuffer(b"abcdefz", dtype=np.uint8), size=int(lens.sum()), p=probs / probs.sum())
    planted = np.frombuffer(b"abcabcabcab", dtype=np.uint8)
    for k in rng.choice(n, n // 25, replace=False):
        s0 = starts[k] + rng.integers(0, lens[k] - len(planted) + 1)
        text[s0:s0 + len(planted)] = planted
    for k in rng.choice(n, n // 50, replace=False):
        text[starts[k] + rng.integers(0, lens[k])] = 0
    off, ln, nbytes = K.arena_layout(lens.astype(np.uint32), 0, n)
    arena = np.zeros(nbytes, dtype=np.uint8)
    arena[np.repeat(off.astype(np.int64) - starts, lens) + np.arange(text.size)] = text
    return arena, off, ln


def test_sliced_reduce_accumulates(gm, oracle):
    """80 000 payloads and 256 blocks per CU: every kernel runs a grid of 20 000 blocks, more than 16 384, so the partial counts
    of a pattern are added up by several reduce blocks that ADD to counts[] -- onto a running total under
    KMPGPU_OPT_ACCUMULATE, onto a counter the scan kernel has put to 0 otherwise (flat and packed kernels), while the fused
    pass and the general kernels overwrite in one slice when they do not accumulate."""
    n = 80_000
    batches = {False: [_small_payload_batch(s, n) for s in (1, 2, 3)], True: [_small_payload_batch(s, n, 96) for s in (4, 5, 6)]}
    wants = {u: [oracle.count(*a, B_PATTERNS, threads=8)[0] for a in bs] for u, bs in batches.items()}
    for ws in wants.values():
        assert all(int(w.min()) > 0 for w in ws) and len({tuple(w.tolist()) for w in ws}) == len(ws)
    try:
        gm.set_patterns(B_PATTERNS)
        gm.set_option(OPT_BLOCKS_PER_CU, 256)
        for mode, kernel in ((MODE_FILTER, KERNEL_FLAT), (MODE_FILTER, KERNEL_PACKED), (MODE_FILTER, KERNEL_FUSED), (MODE_FILTER, KERNEL_GENERAL),
                             (MODE_AUTOMATON, KERNEL_GENERAL)):
            uniform = kernel == KERNEL_FLAT
            bs, ws = batches[uniform], wants[uniform]
            _select(gm, mode, kernel)
            gm.set_option(OPT_ACCUMULATE, 1)
            gm.counts_reset()
            total = np.zeros(len(B_PATTERNS), dtype=np.uint64)
            for a, w in zip(bs, ws):
                gm.load_arena(*a)
                got, t = gm.scan()
                total += w
                assert t.grid_blocks > 16384, (mode, kernel, t.grid_blocks)
                assert got.tolist() == total.tolist(), (mode, kernel, "accumulated")
            got, t = gm.scan()                                       # no reset: the last batch once more
            total += ws[-1]
            assert got.tolist() == total.tolist(), (mode, kernel, "again")
            gm.set_option(OPT_ACCUMULATE, 0)
            got, t = gm.scan()
            assert t.grid_blocks > 16384 and got.tolist() == ws[-1].tolist(), (mode, kernel, "overwrite")

        # offset records at this grid: counts in the pass's own buffer, the running total left as it was
        a, w = batches[False][-1], wants[False][-1]
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        for a0 in batches[False][:2]:
            gm.load_arena(*a0)
            gm.scan()
        running = wants[False][0] + wants[False][1]
        gm.load_arena(*a)
        for fused in (0, 1):
            _select(gm, MODE_FILTER, KERNEL_FUSED if fused else KERNEL_PACKED)
            recs, found, counts = gm.scan_offsets(int(w.sum()) + 10)
            assert found == int(w.sum()) == len(recs) and counts.tolist() == w.tolist(), fused
            assert np.bincount(recs["pattern"].astype(np.int64), minlength=len(B_PATTERNS)).tolist() == w.tolist()
            assert gm.counts_read().tolist() == running.tolist(), fused
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# C. the fused pass's pool when its first group is the wide kernel
# ------------------------------------------------------------------------------------------------
def _pool_patterns(rng):
    """~1 100 distinct patterns of 3-40 bytes over "abc" (a few first-three-byte keys: the classes fill, classed groups form),
    the nine 2-byte ones (a plain first group), two distinct 1-byte riders and duplicates."""
    seen = set()

    def fresh(m):
        while True:
            p = bytes(rng.choice(b"abc") for _ in range(m))
            if p not in seen:
                seen.add(p)
                return p

    two = [bytes([x, y]) for x in b"abc" for y in b"abc"]
    three = [bytes([x, y, z]) for x in b"abc" for y in b"abc" for z in b"abc"]
    four = [bytes([x, y, z, w]) for x in b"abc" for y in b"abc" for z in b"abc" for w in b"abc"]
    seen.update(two + three + four)
    rest = [fresh(5) for _ in range(200)] + [fresh(rng.randrange(6, 41)) for _ in range(800)]
    distinct = three + four + rest
    rng.shuffle(distinct)
    pats = distinct[:500] + two + [b"a", b"z"] + distinct[500:]
    for _ in range(30):
        pats.insert(rng.randrange(len(pats) + 1), rng.choice(pats))
    return pats


def _pool_arena(rng_np, planted, n=48):
    """n payloads of 20-150 KB over "abcd" ('d' over half of it, a little 'z'), planted copies of long patterns, a 0x00 in a
    third of them."""
    lens = rng_np.integers(20_000, 150_001, n)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    probs = np.array([0.15, 0.15, 0.15, 0.545, 0.005])
    text = rng_np.choice(np.frombuffer(b"abcdz", dtype=np.uint8), size=int(lens.sum()), p=probs)
    for _ in range(3000):
        p = planted[int(rng_np.integers(len(planted)))]
        k = int(rng_np.integers(n))
        s0 = starts[k] + int(rng_np.integers(0, lens[k] - len(p) + 1))
        text[s0:s0 + len(p)] = np.frombuffer(p, dtype=np.uint8)
    for k in range(0, n, 3):
        text[starts[k] + int(rng_np.integers(lens[k] * 3 // 4, lens[k]))] = 0
    blob = text.tobytes()
    return [blob[s:s + L] for s, L in zip(starts.tolist(), lens.tolist())]


def test_fused_pool_with_riders_and_classed_groups(gm, oracle):
    """The fused pass's work units are planned for the kernel of its FIRST group: with 1-byte patterns riding along that is
    the wide kernel, 12-wavefront blocks, so a region's plan has 2 x 12 = 24 own units.  The later groups here are classed
    ones and run 16-wavefront blocks against that plan: their n_own is 32, the units 24-31 are some wavefront's own share
    for them and their pool starts at unit 32 (a region of 32 units or fewer gets no pool counter).
    48 payloads, 3.98 MB: a grid of 12 4-wavefront blocks = 4 wide blocks = 2 regions of 1.9 MiB, each with a pool (regions of
    1 MiB and more), 24 own units of 40 KiB and 985 KiB left for the pool:  OPT_FUSED_UNIT 0 -> 50 pool units of 20 KiB (74
    units a region), 1024 -> 197 of 5 KiB (221, the LDS limit on a block's units), 32 KiB -> 31 (55), 1 MiB -> 1 (25: for the
    classed groups no pool at all, unit 24 is the own share of their 25th wavefront).  (The packet count bounds the grid:
    KMPGPU_OPT_BLOCKS_PER_CU does not change it here.)  The same once more with dirty slot padding on a borrowed arena, where every group is the wide kind."""
    rng = random.Random(1500)
    pats = _pool_patterns(rng)
    planted = [p for p in pats if len(p) >= 9][:300]
    payloads = _pool_arena(np.random.default_rng(1500), planted)
    arena = K.HostArena.from_payloads(payloads)
    want, _ = oracle.count(arena.bytes, arena.off, arena.len, pats, threads=8)
    assert int(np.count_nonzero(want)) > len(pats) // 3 and all(want[pats.index(p)] > 0 for p in (b"a", b"z", planted[0]))
    units = (0, 1024, 32768, 1 << 20)
    try:
        gm.set_patterns(pats)
        _select(gm, MODE_FILTER, KERNEL_FUSED)
        gm.load_arena(arena)
        for unit in units:
            gm.set_option(OPT_FUSED_UNIT, unit)
            got, t = gm.scan()
            assert t.grid_blocks == 12, t.grid_blocks            # the region arithmetic of the docstring
            assert t.launches >= 3, t.launches                   # a plain first group and classed ones
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (unit, [(pats[int(i)], int(got[i]), int(want[i])) for i in bad[:5]])
        gm.set_option(OPT_FUSED_UNIT, 0)
        recs, found, counts = gm.scan_offsets(int(want.sum()) + 10)
        assert found == int(want.sum()) == len(recs) and counts.tolist() == want.tolist()
        _check_records(recs, arena, pats, want)
        del recs

        # borrowed, padding left dirty: the bytes behind every payload continue its text, so a kernel that read past the
        # payload's length would count more
        dirty = arena.bytes.copy()
        end = np.append(arena.off[1:], arena.bytes.size).astype(np.int64)
        for o, ln, e in zip(arena.off.astype(np.int64), arena.len.astype(np.int64), end):
            dirty[o + ln:e] = np.frombuffer((b"abc" * ((e - o - ln) // 3 + 1))[:e - o - ln], dtype=np.uint8)
        d_arena = torch.from_numpy(dirty).cuda()
        d_off = torch.from_numpy(arena.off.astype(np.int64)).cuda()
        d_len = torch.from_numpy(arena.len.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        gm.attach_arena(d_arena, d_off, d_len)
        for unit in units:
            gm.set_option(OPT_FUSED_UNIT, unit)
            got, t = gm.scan()
            assert got.tolist() == want.tolist(), ("dirty", unit)
        gm.load_arena(arena)
        del d_arena, d_off, d_len
    finally:
        reset(gm)
