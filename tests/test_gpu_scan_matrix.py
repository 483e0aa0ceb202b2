"""Every scan-kernel instantiation the dispatch can select, run once against the CPU oracle and the host model on a real MI355X.

tests/scan_matrix.py names the 98 instantiations and the options, arena, pattern set and call that launch each;
tests/test_scan_matrix_host.py holds that table to what the compiler emits.  Here every row is one case of `test_row`: run_case sets the
row's options, loads the arena, sets the patterns and compares the call's outputs exactly -- counts with the CPU oracle, hit matrices
and offset records with tests/match_model.py.  test_trace_names_every_row runs the same cases in a fresh process under a kernel trace
and shows that the kernels traced are the kernels the rows name, all of them and no other.

Inputs (built once per module, shared by all rows; the borrowed arenas hold the same payloads as the library's own ones, with text in
their padding, so they share the expectations too):
  uniform   320 payloads of 2309 bytes (slots of 2320).  line_quantum(2320) = 8 and 6144 / 2320 / 8 * 8 = 0, so grid_blocks gives the flat
            kernel ranges of 8 payloads = 18 560 bytes under the default grid; under KMPGPU_OPT_BLOCKS_PER_CU = 1 enqueue_set rounds the one
            payload per wavefront up to the same 8.  A range's chunks start at its first byte, so the 1 KiB boundaries fall at another
            place in each of its payloads.
  mixed     1060 payloads: 0..599 bytes (some empty, some a multiple of 16, some one short of it), and 25 of 8300..11 600 bytes; the long
            ones at k = 0, 53, 106, .. and at k = 1024, 1032, .. so that under BLOCKS_PER_CU = 1 (1024 wavefronts) a wavefront of the
            general kernel goes from one long payload to another.
Range length against DEPTH, read off the launch code:
  flat      19 chunks per range (18 560 bytes), both grids: the ring fills and wraps at every depth, 8 included.  (With the 1500-byte
            payloads of the benchmark a range is 6 chunks and depth 8 never fills; that shape is not taken here.)
  packed    default grid: span / (4 x 16 KiB) = 9 blocks, 36 wavefronts of 16 chunks: wraps at depths 3, 4 and 6.  BLOCKS_PER_CU = 1: 1024
            wavefronts of about 560 bytes, ranges of one or two payloads -- one chunk, the ring never fills -- except where a long payload
            is a range of its own: 9..12 chunks, wraps at every depth.
  general   a wavefront's ring runs on over its payloads (k, k + 4 x blocks, ..).  Default grid: 265 blocks, one payload per wavefront:
            the ring fills and wraps only in the 25 long payloads (9..12 chunks against DEPTH + 2 <= 8), every other wavefront has one chunk.
            BLOCKS_PER_CU = 1: 256 blocks, wavefronts 0..35 have two payloads (k and k + 1024): wavefront 0 two long ones, wavefronts 8,
            16, 24 and 32 a short one and then a long one, so the ring runs from one payload into the next.
  fused     DEPTH = 3.  span / (4 x 2 KiB) = 69 blocks of four wavefronts -> 8 regions of 70 KiB (11 of 51 KiB for the wide kernels), no
            pool, work units of 3 chunks: the ring fills and does not wrap, except in the units that hold a long payload (units are cut at
            payload starts): 9..12 chunks and more.  Longer units need an arena of 16 MiB and more; the plan does not permit them here.
Text: six common letters of both cases and five rare bytes, with occurrences of the long patterns planted across every 1 KiB boundary
of a payload, across 16-byte lane boundaries, at a payload's last byte, and cut in two by a payload's end -- in the borrowed arenas the
padding behind it holds the rest, so a kernel that reads past L_k counts too many.  Every third payload has 0x00 bytes: the first one
directly before, inside or directly behind a planted occurrence, further ones behind it.

Placed rows: test_row_placed runs every row again with its arena attached inside one borrowed buffer of a little over 4 GiB
(gpu_support.attach_placed) at the placements `split`, `edge` and `behind` of gpu_support.placed_base -- 2^32 inside payload SPLIT_K, 48
bytes of it in front; a slot that ends at 2^32 with EDGE_K starting there; every offset above 2^32 -- with the same expectations and
under both grids.  The *_dirty kinds keep their text-filled padding, the others get zero padding, which the padding check over the high
arena has to find clean for the row's kernel to run: test_trace_names_every_row_behind holds the traced kernels to the rows' names once
more.  Inputs._plant_for_placements puts occurrences around byte 48 of SPLIT_K, at the head of EDGE_K and at the end of EDGE_K - 1;
Inputs.placement_facts asserts on the CPU that every pattern set has a match across 2^32 under `split` and matches on either side of it
under `edge`.  tests/test_gpu_high_offsets.py has the reasons, the kernels behind the marking pass and the record of what these cases
catch.

Run on a real MI355X:  python -m pytest tests/test_gpu_scan_matrix.py -m gpu
Measured there: the 98 rows and the trace test, 99 passed in 16 s (the trace test 8.3 s, the slowest row 1.2 s: a classed set's 140 000
offset records, sorted and compared on the host).  With the 294 placed rows and the second trace: 394 passed in 32 s (each trace 8.1 s,
the slowest row 1.1 s, the slowest placed row 0.54 s).

Checked to bite: three memory-safe changes made to a scratch build (never committed), one per file, each inside `if constexpr` so that
one instantiation alone is changed.  With all three in one library these rows failed, every other row passed, and the rest of the GPU
suite (874 tests, this module left out) passed:
  kmp_scan_stream_kernels.inc, `DEPTH == 6 && !NT && !EMIT` of the flat kernel: the candidates of a range's last chunk are dropped --
      kmp_scan_flat_kernel<6, false, false> (all six patterns short, e.g. 4517 of 4550);
  kmp_scan_general.hip, `DEPTH == 5 && MASKED && MODE == 0 && !NT && !WHOLE`: a start of a pattern of up to 4 bytes counts only where
      s + m < E instead of <= E -- kmp_scan_kernel<5, true, 0, false, false> (the four short patterns, e.g. 10 685 of 10 708);
  kmp_scan_multi.hip, `!NT && CLEAN && !ONES && !CLASSED && !WHOLE && !EMIT` in count_match: a match that starts in a lane's last byte
      is not counted -- kmp_scan_multi_kernel<3, false, true, false, false> (every pattern about a sixteenth short), and
      kmp_scan_multi_kernel<3, false, true, false, true>, whose classed set runs that kernel for its plain first group (`also`).
"""
import csv
import glob
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

from gpu_support import (PLACEMENTS, SPLIT_FRONT, attach_placed, big_buffer, check_offsets, check_packets, gm, load, make_big_buffer,  # noqa: E402,F401
                         placed_base, reset)  # (torch first; big_buffer, gm: fixtures; make_big_buffer: for tests/scan_matrix_child.py)

import match_model as MM  # noqa: E402
import scan_matrix as SM  # noqa: E402
from multithreading_string_matching_amd.matcher import OPT_BLOCKS_PER_CU  # noqa: E402

COMMON, RARE = b"abcdAB", b"-eE\x80\x01"
UNIFORM_N, UNIFORM_LEN = 320, 2309
MIXED_N = 1060
LONG_LENGTHS = (4, 5, 8, 9, 16, 17, 40, 99)
GRIDS = (0, 1)                                          # KMPGPU_OPT_BLOCKS_PER_CU: the default grid, and one block per CU
# The payloads the placements of gpu_support.placed_base are hung on, in both payload sets: SPLIT_K straddles 2^32 under `split`
# (no multiple of 64, more than 64 payloads behind it), EDGE_K starts at 2^32 under `edge`.  Neither they nor EDGE_K - 1 hold a 0x00
# (k % 3 != 0), so both text-end rules see their plants.
SPLIT_K, EDGE_K = 101, 110
STRADDLER = 4                                           # of LONG_LENGTHS: in the sets "long" and "riders"; it holds "ab", of "short" and "classed"


def _text(nrng, n):
    p = np.array([0.16] * len(COMMON) + [0.008] * len(RARE))
    return bytearray(nrng.choice(np.frombuffer(COMMON + RARE, dtype=np.uint8), size=n, p=p).tobytes())


def _mixed_length(rng, k):
    if k % 53 == 0 or (k >= 1024 and k % 8 == 0):
        return 8300 + (k * 977) % 3300
    if k % 97 == 5:
        return 0
    L = rng.randrange(1, 600)
    return L - L % 16 if k % 7 == 0 and L >= 16 else L | 15 if k % 7 == 1 else L


def _payload(rng, nrng, k, L, plants):
    """(payload, what its padding is to begin with)"""
    b = _text(nrng, L)
    planted = []

    def plant(p, s):
        if 0 <= s and s + len(p) <= L:
            b[s:s + len(p)] = p
            planted.append((s, len(p)))
    for j in range(1, L // 1024 + 1):                   # across every 1 KiB boundary of the payload
        p = plants[(k + j) % len(plants)]
        plant(p, j * 1024 - len(p) // 2)
    for _ in range(L // 150 + 1):
        p = rng.choice(plants)
        if L >= len(p):
            plant(p, rng.randrange(L - len(p) + 1))
        p = rng.choice(plants)                          # across a lane boundary
        plant(p, 16 * rng.randrange(1, L // 16 + 2) - rng.randrange(1, len(p)))
    if k % 3 == 0 and planted:
        s, m = planted[rng.randrange(len(planted))] if L < 4000 or k % 2 else min(planted)
        first = (s - 1, s + m // 2, s + m)[(k // 3) % 3]  # directly before, inside, directly behind
        if 0 <= first < L:
            b[first] = 0
        for s, m in rng.sample(planted, min(3, len(planted))):      # text bytes under whole payloads
            for z in (s - 1, s + m):
                if first < z < L:
                    b[z] = 0
    pad = (-L) % 16 or (16 if L == 0 else 0)
    cont = b""
    if k % 4 == 1:                                      # a match that ends with the payload
        p = rng.choice(plants)
        plant(p, L - len(p))
    elif k % 4 == 2 and pad:                            # an occurrence cut in two by the payload's end
        p = rng.choice(plants)
        c = len(p) - min(pad, len(p) - 1)
        if c <= L:
            b[L - c:] = p[:c]
            cont = p[c:]
    return bytes(b), cont


class Inputs:
    """The two payload sets, their borrowed twins' slots, the four pattern sets, and every expectation, computed when first asked for."""

    def __init__(self, oracle):
        self.oracle = oracle
        rng, nrng = random.Random(20260), np.random.default_rng(20260)
        self.long = [bytes(_text(nrng, m)) for m in LONG_LENGTHS]
        self.payloads, self.slots = {}, {}
        for name, lens in (("uniform", [UNIFORM_LEN] * UNIFORM_N), ("mixed", [_mixed_length(rng, k) for k in range(MIXED_N)])):
            built = [_payload(rng, nrng, k, L, self.long) for k, L in enumerate(lens)]
            self._plant_for_placements(built)
            self.payloads[name] = [t for t, _ in built]
            slots = []
            for t, cont in built:
                pad = (-len(t)) % 16 or (16 if not t else 0)
                fill = bytes(_text(nrng, pad))
                slots.append(t + (cont + fill)[:pad])
            self.slots[name] = slots
        texts = [t[:MM.text_end(t)] for t in self.payloads["mixed"] if MM.text_end(t) >= 8]
        cut, seen = [], set(self.long)
        while len(cut) < 300:                           # pieces of the text the strlen rule sees, so that every one matches under both rules
            t = rng.choice(texts)
            m = rng.choice((3, 5, 6, 7, 8, 8, 6, 5))
            s = rng.randrange(len(t) - m + 1)
            if t[s:s + m] not in seen:
                seen.add(t[s:s + m])
                cut.append(t[s:s + m])
        L = self.long
        self.sets = {"long": list(L),
                     "short": [b"-", b"ab", b"Bca", b"dA", L[0], L[5], L[7]],
                     "riders": [b"-", L[1], b"E", L[3], L[4], b"\x80", b"cab", b"Ad"],
                     "classed": [b"ab", b"Bd"] + cut + [L[2], L[5], L[6]]}
        self._counts, self._starts, self._facts = {}, {}, set()

    def _plant_for_placements(self, built):
        """SPLIT_K: long[5] up to byte 44 and long[STRADDLER] from byte 45 on, whose bytes 2 and 3 -- "ab" -- are the payload's bytes 47 and
        48: under `split` that occurrence and that "ab" hold the last byte in front of 2^32 and the first one behind it.  (Two occurrences
        cannot both hold byte 47: the second one ends directly in front of the first.)  EDGE_K starts with long[STRADDLER] and EDGE_K - 1 ends
        with it: under `edge` a match from byte 2^32 on and one up to byte 2^32 - 1, the last byte of a payload that fills its slot or not."""
        Y, X = self.long[STRADDLER], self.long[5]
        assert Y[2:4] == b"ab" and Y.endswith(b"-")

        def put(k, at, p):
            t, cont = built[k]
            at = at if at >= 0 else len(t) + at
            assert 0 <= at and at + len(p) <= len(t) and 0 not in t
            built[k] = (t[:at] + p + t[at + len(p):], cont)
        put(SPLIT_K, SPLIT_FRONT - 3 - len(X), X)
        put(SPLIT_K, SPLIT_FRONT - 3, Y)
        put(EDGE_K, 0, Y)
        put(EDGE_K - 1, -len(Y), Y)
        if (EDGE_K - 1) % 4 == 2:                       # (its padding would go on with the occurrence cut by its end)
            built[EDGE_K - 1] = (built[EDGE_K - 1][0], b"")

    def placement_facts(self, row, placement):
        """Under `split` the row's pattern set has a match that contains byte 2^32 and the byte in front of it; under `edge` one that
        starts in the first lane behind 2^32 and one that ends in the last lane in front of it -- for the long patterns a match from a
        payload's byte 0 at 2^32 on, and one that ends with the payload in front of it."""
        whole = bool(row["options"].get("WHOLE_PAYLOAD", 0))
        pats, _ = self.patterns(row)
        st = self.starts(row, whole)
        payloads = self.payloads[self.base(row["arena"])]

        def spans(k):
            return [(s, s + len(pats[i])) for i, ss in enumerate(st[k]) for s in ss]
        if placement == "split":
            assert any(s < SPLIT_FRONT < e for s, e in spans(SPLIT_K)), row["name"]
        elif placement == "edge":
            L = len(payloads[EDGE_K - 1])
            assert any(s < 16 for s, _ in spans(EDGE_K)) and any(e > L - 16 for _, e in spans(EDGE_K - 1)), row["name"]
            if row["patterns"] in ("long", "riders"):
                assert any(s == 0 for s, _ in spans(EDGE_K)) and any(e == L for _, e in spans(EDGE_K - 1)), row["name"]

    @staticmethod
    def base(arena):
        return "uniform" if arena.startswith("uniform") else "mixed"

    @staticmethod
    def borrowed(arena):
        return arena.endswith("dirty")

    def patterns(self, row):
        pats = self.sets[row["patterns"]]
        return pats, ([i % 2 == 1 for i in range(len(pats))] if row["nocase"] else None)

    def counts(self, row, whole):
        key = (self.base(row["arena"]), row["patterns"], row["nocase"], whole)
        if key not in self._counts:
            pats, nocase = self.patterns(row)
            self._counts[key] = MM.oracle_counts(self.oracle, self.payloads[key[0]], pats, nocase, whole)
        return self._counts[key]

    def starts(self, row, whole, windows=None):
        key = (self.base(row["arena"]), row["patterns"], row["nocase"], whole, windows is not None)
        if key not in self._starts:
            pats, nocase = self.patterns(row)
            self._starts[key] = MM.starts(self.payloads[key[0]], pats, windows=windows, nocase=nocase, whole=whole)
        return self._starts[key]

    def windows(self, row):
        """a window on two patterns of the row's set"""
        w = [(0, None)] * len(self.sets[row["patterns"]])
        w[0], w[-1] = (40, 300), (0, 30)
        return w

    def assert_facts(self, row):
        """what a case asserts on the CPU before anything runs on the device"""
        whole = bool(row["options"].get("WHOLE_PAYLOAD", 0))
        pats, nocase = self.patterns(row)
        mine, other = self.counts(row, whole), self.counts(row, not whole)
        assert all(c > 0 for c in mine), [(p, c) for p, c in zip(pats, mine) if c == 0][:6]
        # the two text-end rules tell this input apart (every kernel family has a _whole twin), for most of the patterns
        strlen, full = (other, mine) if whole else (mine, other)
        assert all(f >= s for f, s in zip(full, strlen)) and 2 * sum(f > s for f, s in zip(full, strlen)) > len(pats), row["name"]
        base = self.base(row["arena"])
        payloads, slots = self.payloads[base], self.slots[base]
        assert (len({len(t) for t in payloads}) == 1) == row["arena"].startswith("uniform")
        key = (base, row["patterns"], row["nocase"])
        if self.borrowed(row["arena"]) and key not in self._facts:
            pad = b"".join(s[len(t):] for t, s in zip(payloads, slots))
            assert len(pad) > len(payloads) and 0 not in pad
            assert all(len(s) % 16 == 0 and len(s) >= 16 and s.startswith(t) for t, s in zip(payloads, slots))
            # the padding continues occurrences that a payload's end cuts: read as text, the slots hold more matches than the payloads
            over = MM.oracle_counts(self.oracle, slots, pats, nocase, True)
            full = self.counts(row, True)
            assert all(o >= f for o, f in zip(over, full)) and sum(o > f for o, f in zip(over, full)) >= min(3, len(pats) // 2), row["name"]
            self._facts.add(key)
        if row["call"] == "scan_packets":               # the windows of the second run change the hits of their two patterns
            hits, hits_w = MM.hits(self.starts(row, whole)), MM.hits(self.starts(row, whole, self.windows(row)))
            assert (hits[0] != hits_w[0]).any() and (hits[-1] != hits_w[-1]).any() and (hits[1:-1] == hits_w[1:-1]).all(), row["name"]


@pytest.fixture(scope="module")
def inputs(oracle):
    return Inputs(oracle)


def run_case(gm, row, inputs, placement="low", buf=None):
    """placement "low": the arena as the row names it, the library's own copy or a borrowed one.  Every other placement of
    gpu_support.PLACEMENTS: a borrowed arena inside buf (gpu_support.big_buffer) at absolute offsets around 2^32 -- the *_dirty kinds with
    their text-filled padding, the others with zero padding, which kmp_check_padding_kernel over the high arena has to find clean for the
    row's kernel to be the one that runs."""
    whole = bool(row["options"].get("WHOLE_PAYLOAD", 0))
    inputs.assert_facts(row)
    inputs.placement_facts(row, placement)
    pats, nocase = inputs.patterns(row)
    counts = inputs.counts(row, whole)
    base = inputs.base(row["arena"])
    reset(gm)
    try:
        for key, value in row["options"].items():
            gm.set_option(SM.OPTIONS[key], value)
        slots = inputs.slots[base] if inputs.borrowed(row["arena"]) else None
        if placement == "low":
            keep = load(gm, inputs.payloads[base], slots)
        else:
            at = placed_base(placement, inputs.payloads[base], slots, {"split": SPLIT_K, "edge": EDGE_K}.get(placement))
            keep = attach_placed(gm, inputs.payloads[base], slots, at, buf)
        gm.set_patterns(pats, nocase=nocase if nocase else False)
        for bpc in GRIDS:
            gm.set_option(OPT_BLOCKS_PER_CU, bpc)
            if row["call"] == "scan":
                got = gm.scan()[0].tolist()
                assert got == counts, (row["name"], bpc, [(pats[i], g, w) for i, (g, w) in enumerate(zip(got, counts)) if g != w][:6])
                continue
            st = inputs.starts(row, whole)
            # an emitting kernel marks hits for kmpgpu_scan_packets and writes records for kmpgpu_scan_offsets: the row's call under both
            # grids, the other one under the second
            for call in (row["call"],) + ((("scan_packets", "scan_offsets")[row["call"] == "scan_packets"],) if bpc else ()):
                if call == "scan_packets":
                    check_packets(gm, MM.hits(st), counts)
                else:
                    check_offsets(gm, MM.records(st), counts)
        if row["call"] == "scan_packets":               # once more with a window on two patterns: other hits, the same totals
            w = inputs.windows(row)
            gm.set_windows(w)
            check_packets(gm, MM.hits(inputs.starts(row, whole, w)), counts)
            gm.set_windows(None)
        del keep
    finally:
        reset(gm)


@pytest.mark.parametrize("row", SM.ROWS, ids=[r["name"] for r in SM.ROWS])
def test_row(gm, inputs, row):
    run_case(gm, row, inputs)


def test_trace_names_every_row(tmp_path):
    """The same cases in a fresh process (tests/scan_matrix_child.py) under a kernel trace: the scan kernels that ran are the rows' names,
    every one of them, and none the table calls unreachable.  With tests/test_scan_matrix_host.py: every instantiation the launchers
    can pick ran inside a case that compares its results."""
    _trace_names_every_row(tmp_path, "low")


def test_trace_names_every_row_behind(tmp_path):
    """The same with every arena placed behind 2^32 (the child makes a buffer of its own; this module's is not made yet): a placed row
    runs the instantiation it names, not another one that happens to count the same -- the padding check over the high arena decides as
    it does for the library's own copy."""
    _trace_names_every_row(tmp_path, "behind")


def _trace_names_every_row(tmp_path, placement):
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None:
        pytest.skip("rocprofv3 not installed")
    out = str(tmp_path / "trace")
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.join(ROOT, "tests", "scan_matrix_child.py"), placement],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert files, (os.listdir(out) if os.path.isdir(out) else out, r.stderr[-2000:])
    traced = set()
    for path in files:
        with open(path, newline="") as f:
            for rec in csv.DictReader(f):
                name = SM.normalise(rec["Kernel_Name"])
                if SM.is_scan_kernel(name):
                    traced.add(name)
    rows = {row["name"] for row in SM.ROWS}
    assert not traced & set(SM.UNREACHABLE), sorted(traced & set(SM.UNREACHABLE))
    assert traced == rows, ("rows whose kernel never ran: %s" % sorted(rows - traced), "kernels no row names: %s" % sorted(traced - rows))


# behind the trace tests: the buffer of this module is made when the first placed row asks for it, after the child processes have had
# theirs
@pytest.mark.parametrize("placement", PLACEMENTS[1:])
@pytest.mark.parametrize("row", SM.ROWS, ids=[r["name"] for r in SM.ROWS])
def test_row_placed(gm, inputs, big_buffer, row, placement):
    run_case(gm, row, inputs, placement, big_buffer)
