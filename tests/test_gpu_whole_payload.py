"""Whole-payload scanning (KMPGPU_OPT_WHOLE_PAYLOAD = 1: E_k = L_k, a 0x00 is a text byte like any other) on a real MI355X.

The checker is the CPU oracle, unchanged (it implements the reference's strlen() rule), on the 0x00 bytes mapped to a byte that no
pattern holds (oracle_counts_arena of tests/match_model.py, which says why that is the same count).  Offsets and hit bitmaps are
checked against the host model there.  Every randomised test first asserts, on the CPU, that its input tells the two rules apart.

Run on a real MI355X:  python -m pytest tests/test_gpu_whole_payload.py -m gpu
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

from gpu_support import VARIANTS, gm, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import torch  # noqa: E402

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_FLAT, KERNEL_GENERAL, KERNEL_PACKED, OPT_ACCUMULATE, OPT_BLOCKS_PER_CU, OPT_DEPTH, OPT_FUSED, OPT_FUSED_UNIT, OPT_KERNEL,
    OPT_MODE, OPT_REPACK, OPT_WHOLE_PAYLOAD)

TEXT = b"abcdeABCDE-" + bytes([0x01, 0x80, 0xC1, 0xFE])          # the text alphabet: no 0x00, no MM.REMAP
FIXTURE_KEYS = ["udp.pcap:udp", "udp_1000.pcap:udp", "big_udp.pcap:udp", "very_big_udp.pcap:udp",
                "tcp.pcap:tcp", "tcp.pcap:udp", "udp.pcap:tcp", "udp_1000.pcap:tcp"]
LENGTHS = [1, 2, 3, 4, 8, 9, 16, 17, 40, 99]


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def rand_text(rng, n):
    return bytes(rng.choice(TEXT) for _ in range(n))


def cut_patterns(rng, texts, lengths, per=2):
    pats = []
    for m in lengths:
        for _ in range(per):
            for _ in range(200):
                t = texts[rng.randrange(len(texts))]
                if len(t) >= m:
                    s = rng.randrange(len(t) - m + 1)
                    if 0 not in t[s:s + m]:
                        pats.append(bytes(t[s:s + m]))
                        break
            else:
                pats.append(rand_text(rng, m))
    return pats


def nul_payloads(rng, n, length, pats):
    """Random text with occurrences of `pats` planted in it, then several 0x00 per payload: at byte 0, at the last byte, directly
    before / directly behind / inside a planted occurrence, a run of 16..40, a run of 1024..1100 (a whole chunk of zeros in
    mid-payload), and none at all."""
    out = []
    for k in range(n):
        L = length if length is not None else rng.randrange(0, 2200)
        b = bytearray(rand_text(rng, L))
        planted = []
        for _ in range(rng.randrange(1, 6)):
            p = pats[rng.randrange(len(pats))]
            if len(p) <= L:
                s = rng.randrange(L - len(p) + 1)
                b[s:s + len(p)] = p
                planted.append((s, len(p)))
        kinds = rng.sample(["first", "last", "before", "behind", "inside", "run16", "run1024"], 3) if rng.random() < 0.9 else []
        for kind in kinds if L else []:
            s, m = planted[rng.randrange(len(planted))] if planted else (rng.randrange(L), 1)
            if kind == "first":
                b[0] = 0
            elif kind == "last":
                b[L - 1] = 0
            elif kind == "before" and s > 0:
                b[s - 1] = 0
            elif kind == "behind" and s + m < L:
                b[s + m] = 0
            elif kind == "inside":
                b[s + rng.randrange(m)] = 0
            elif kind == "run16":
                a = rng.randrange(L)
                z = min(L - a, rng.randrange(16, 41))
                b[a:a + z] = bytes(z)
            elif kind == "run1024" and L >= 1300:
                a = rng.randrange(40, L - 1150)
                z = rng.randrange(1024, 1101)
                b[a:a + z] = bytes(z)
        out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def whole_golden():
    with open(os.path.join(GOLDEN, "whole_payload_counts.json")) as f:
        return json.load(f)["fixtures"]


def select(gm, variant):
    _, mode, kernel, fused = variant
    gm.set_option(OPT_MODE, mode); gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)


# ------------------------------------------------------------------------------------------------
# 1. every kernel family
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_kernel_family(gm, oracle, uniform, variant):
    rng = random.Random(211 + 7 * uniform + len(variant[0]))
    texts = [rand_text(rng, 400) for _ in range(20)]
    pats = cut_patterns(rng, texts, LENGTHS) + [b"a", b"-", b"\xc1", b"\x01"]      # 1-byte patterns ride along with the fused pass
    payloads = nul_payloads(rng, 600, 1500 if uniform else None, pats)
    assert sum(1 for p in payloads if p.count(0) >= 2) > 300 and any(bytes(1024) in p for p in payloads) and any(0 not in p for p in payloads)
    arena = K.HostArena.from_payloads(payloads)
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True)
    strlen = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats)
    assert whole != strlen and all(w >= s for w, s in zip(whole, strlen))
    assert whole == MM.counts(MM.starts(payloads, pats, whole=True))             # the identity itself, on this input
    assert sum(1 for w, s in zip(whole, strlen) if w != s) >= len(LENGTHS)
    reset(gm)
    select(gm, variant)
    gm.set_patterns(pats)
    gm.load_arena(arena)
    for opt, want in ((1, whole), (0, strlen), (1, whole)):                          # the same context, nothing reloaded in between
        gm.set_option(OPT_WHOLE_PAYLOAD, opt)
        got = gm.scan()[0].tolist()
        assert got == want, (variant[0], opt, [(pats[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:6])
    for depth in (2, 3, 5, 6, 8):                                                    # any depth is mapped to an instantiated one, never refused
        gm.set_option(OPT_DEPTH, depth)
        assert gm.scan()[0].tolist() == whole, (variant[0], depth)
    reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. one byte zeroed: the operand whose zero bytes a masked SAD skips must be the pattern, never the text
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_one_byte_zeroed_never_matches(gm, oracle, variant):
    rng = random.Random(5)
    L = 640
    control = b"yzx"                                                                 # occurs in the filler, also behind the 0x00
    reset(gm)
    select(gm, variant)
    everything, all_pats = [], []
    for m in LENGTHS:
        p = bytes(rng.choice(b"abcdeABCDE") for _ in range(m))
        payloads = []
        for j in range(m):
            for front in (rng.randrange(0, 16), 16 * rng.randrange(1, 30), rng.randrange(0, L - m)):
                front = min(front, L - m)
                z = bytearray(p)
                z[j] = 0
                t = (b"xyz" * 300)[:front] + bytes(z) + (b"xyz" * 300)[: L - m - front]
                assert len(t) == L
                payloads.append(t)
        arena = K.HostArena.from_payloads(payloads)
        pats = [p, control]
        whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True)
        strlen = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats)
        assert whole[0] == 0 and whole != strlen
        gm.set_patterns(pats)
        gm.load_arena(arena)
        gm.set_option(OPT_WHOLE_PAYLOAD, 1)
        assert gm.scan()[0].tolist() == whole, (variant[0], m)
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)
        assert gm.scan()[0].tolist() == strlen, (variant[0], m)
        everything += payloads
        all_pats.append(p)
    # all lengths in one set (the fused pass with every pattern in its tables)
    arena = K.HostArena.from_payloads(everything)
    pats = all_pats + [control]
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True)
    assert whole == MM.counts(MM.starts(everything, pats, whole=True))
    gm.set_patterns(pats)
    gm.load_arena(arena)
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    assert gm.scan()[0].tolist() == whole, variant[0]
    reset(gm)


# ------------------------------------------------------------------------------------------------
# 3. payload ends
# ------------------------------------------------------------------------------------------------
def _end_payloads(rng, pats, n, with_empty, multiple_of_16=True):
    """Payloads whose tails and heads hold pieces of the patterns: whole occurrences that end at the last byte, and occurrences cut
    in two by the boundary between payload k and k + 1."""
    lens = []
    for _ in range(n):
        if with_empty and rng.random() < 0.15:
            lens.append(0)
        else:
            lens.append(16 * rng.randrange(1, 14) if multiple_of_16 else rng.randrange(1, 200))
    b = [bytearray(rand_text(rng, L)) for L in lens]
    for k in range(n):
        if lens[k] >= 2 and rng.random() < 0.5:
            b[k][rng.randrange(lens[k] // 2)] = 0                                     # a 0x00 in the first half: the rules differ
    for k in range(n):
        p = pats[rng.randrange(len(pats))]
        m = len(p)
        if rng.random() < 0.4:
            if m <= lens[k]:
                b[k][lens[k] - m:] = p                                               # ends exactly at the payload's last byte
        elif m >= 2 and k + 1 < n:
            c = rng.randrange(1, m)
            if c <= lens[k] and m - c <= lens[k + 1]:
                b[k][lens[k] - c:] = p[:c]                                           # straddles the boundary: not a match
                b[k + 1][:m - c] = p[c:]
    return [bytes(x) for x in b]


@pytest.mark.parametrize("with_empty", [False, True])
def test_payload_ends_without_padding(gm, oracle, with_empty):
    rng = random.Random(31 + with_empty)
    pats = [rand_text(rng, m) for m in (2, 3, 4, 8, 9, 16, 17, 40, 99)] + [b"a", b"E"]
    payloads = _end_payloads(rng, pats, 1500, with_empty)
    assert all(len(p) % 16 == 0 for p in payloads) and (with_empty == any(len(p) == 0 for p in payloads))
    arena = K.HostArena.from_payloads(payloads)
    assert arena.nbytes >= sum(max(16, len(p)) for p in payloads)
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True)
    strlen = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats)
    assert whole != strlen and whole == MM.counts(MM.starts(payloads, pats, whole=True))
    # the input has what it is meant to have: matches that end at a payload's end, and windows across a boundary that would match
    joined = b"".join(payloads)
    assert sum(joined.count(p) for p in pats[:9]) > sum(whole[:9]) and any(t.endswith(p) for t in payloads for p in pats[:9] if t)
    reset(gm)
    gm.set_patterns(pats)
    gm.load_arena(arena)
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    for v in VARIANTS:
        select(gm, v)
        assert gm.scan()[0].tolist() == whole, v[0]
    reset(gm)
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    recs, found, counts = gm.scan_offsets(sum(whole) + 8)
    assert found == sum(whole) and counts.tolist() == whole and MM.triples(recs) == sorted(MM.records(MM.starts(payloads, pats, whole=True)))
    reset(gm)


def _dirty_arena(rng, pats, n, gaps):
    """An arena whose padding (and gaps) CONTINUE the pattern a payload ends with: a window that leaves its payload would match."""
    payloads = _end_payloads(rng, pats, n, True, multiple_of_16=False)
    off = np.zeros(n, dtype=np.uint64)
    pos = 0
    for k in range(n):
        if gaps:
            pos += 16 * rng.randrange(0, 3)
        off[k] = pos
        pos += max(16, (len(payloads[k]) + 15) // 16 * 16)
    arena = np.frombuffer(rand_text(rng, pos + 64), dtype=np.uint8).copy()
    ln = np.array([len(p) for p in payloads], dtype=np.uint32)
    tails = 0
    for k, p in enumerate(payloads):
        o = int(off[k])
        arena[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    for k, p in enumerate(payloads):                         # behind every payload that is followed by padding or a gap: the rest of a pattern
        o = int(off[k]) + len(p)
        nxt = int(off[k + 1]) if k + 1 < n else pos
        q = pats[rng.randrange(len(pats))]
        if nxt > o and len(q) >= 2 and len(p) >= 1:
            c = rng.randrange(1, min(len(q), len(p) + 1))
            cont = q[c:][: nxt - o]
            if 0 not in p[len(p) - c:]:
                arena[o - c:o] = np.frombuffer(q[:c], dtype=np.uint8)
                arena[o:o + len(cont)] = np.frombuffer(cont, dtype=np.uint8)
                tails += len(cont) == len(q) - c
    payloads = [bytes(arena[int(off[k]):int(off[k]) + int(ln[k])]) for k in range(n)]
    return arena, off, ln, payloads, tails


@pytest.mark.parametrize("gaps", [False, True])
def test_payload_ends_with_dirty_padding(gm, oracle, gaps):
    """Attached device arenas whose padding continues the pattern: packed (the streaming kernels take the end from the index) and,
    with gaps and KMPGPU_OPT_REPACK = 0, scanned in place by the general kernel; the offsets / packets calls pack it once."""
    rng = random.Random(77 + gaps)
    pats = [rand_text(rng, m) for m in (2, 3, 4, 8, 9, 16, 17, 40)] + [b"b"]
    arena, off, ln, payloads, tails = _dirty_arena(rng, pats, 1200, gaps)
    assert tails > 100                                      # complete occurrences that run out of their payloads: none may count
    whole = MM.oracle_counts_arena(oracle, arena, off, ln, pats, whole=True)
    strlen = MM.oracle_counts_arena(oracle, arena, off, ln, pats)
    st = MM.starts(payloads, pats, whole=True)
    model = sorted(MM.records(st))
    assert whole != strlen and whole == MM.counts(st)
    d_arena = torch.from_numpy(arena).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    gm.set_stream(None)
    reset(gm)
    gm.set_patterns(pats)
    for repack in ((1, 0) if gaps else (1,)):
        gm.set_option(OPT_REPACK, repack)
        gm.attach_arena(d_arena, d_off, d_len)
        for v in VARIANTS:
            select(gm, v)
            for opt, want in ((1, whole), (0, strlen)):
                gm.set_option(OPT_WHOLE_PAYLOAD, opt)
                assert gm.scan()[0].tolist() == want, (gaps, repack, v[0], opt)
        select(gm, VARIANTS[0])
        gm.set_option(OPT_WHOLE_PAYLOAD, 1)
        recs, found, counts = gm.scan_offsets(len(model) + 8)
        assert found == len(model) and counts.tolist() == whole and MM.triples(recs) == model, (gaps, repack)
        r = gm.scan_packets(hits=True)
        assert r["counts"].tolist() == whole and int(r["hits"].sum()) == len({(k, i) for k, _, i in model}), (gaps, repack)
        assert gm.scan()[0].tolist() == whole
    reset(gm)
    assert np.array_equal(d_arena.cpu().numpy(), arena)     # the borrowed arena was never written
    del d_arena, d_off, d_len


# ------------------------------------------------------------------------------------------------
# 4. fused specifics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pats", [300, 1100])
def test_fused_classed_groups_and_pool(gm, oracle, n_pats):
    rng = random.Random(n_pats)
    texts = [rand_text(rng, 300) for _ in range(60)]
    pats = cut_patterns(rng, texts, [rng.randrange(2, 14) for _ in range(n_pats)], per=1)
    pats = list(dict.fromkeys(pats))
    while len(pats) < n_pats:                                 # n_pats DISTINCT patterns
        p = rand_text(rng, rng.randrange(4, 12))
        if p not in pats:
            pats.append(p)
    pats = pats[:n_pats] + pats[:5] + [pats[7]]               # duplicates keep identical counts, one per index
    payloads = nul_payloads(rng, 700, None, pats[:200])
    arena = K.HostArena.from_payloads(payloads)
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True, threads=8)
    strlen = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, threads=8)
    assert whole != strlen and whole[:5] == whole[n_pats:n_pats + 5] and whole[7] == whole[-1]
    reset(gm)
    gm.set_patterns(pats)
    gm.load_arena(arena)
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    for fused, unit in ((1, 0), (1, 1024), (0, 0)):
        gm.set_option(OPT_FUSED, fused); gm.set_option(OPT_FUSED_UNIT, unit)
        assert gm.scan()[0].tolist() == whole, (fused, unit)
    gm.set_option(OPT_FUSED, 1); gm.set_option(OPT_FUSED_UNIT, 1024); gm.set_option(OPT_WHOLE_PAYLOAD, 0)
    assert gm.scan()[0].tolist() == strlen
    reset(gm)


def test_fused_pool_on_a_large_arena(gm, oracle):
    """Regions of more than 1 MiB, so that the pool of work units runs (KMPGPU_OPT_FUSED_UNIT = 1024: a unit per KiB)."""
    rng = random.Random(8)
    texts = [rand_text(rng, 400) for _ in range(20)]
    pats = cut_patterns(rng, texts, [2, 3, 4, 5, 8, 9, 17, 40], per=2) + [b"a", b"\x80"]
    base = nul_payloads(rng, 400, None, pats)
    payloads = [base[rng.randrange(len(base))] for _ in range(60_000)]
    arena = K.HostArena.from_payloads(payloads)
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True, threads=8)
    strlen = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, threads=8)
    assert whole != strlen
    reset(gm)
    gm.set_patterns(pats)
    gm.load_arena(arena)
    gm.set_option(OPT_FUSED, 1)
    gm.set_option(OPT_BLOCKS_PER_CU, 1)                       # few, large regions
    for unit in (1024, 0, 65536):
        gm.set_option(OPT_FUSED_UNIT, unit)
        gm.set_option(OPT_WHOLE_PAYLOAD, 1)
        assert gm.scan()[0].tolist() == whole, unit
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)
        assert gm.scan()[0].tolist() == strlen, unit
    reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. with nocase
# ------------------------------------------------------------------------------------------------
def test_with_nocase_mixed_flags(gm, oracle):
    rng = random.Random(12)
    words = [b"Host", b"hOsT", b"GET", b"User-Agent", b"ab", b"\xc1\xda", b"abcdeABCDEabcdeABCDE"]
    pats = [b"Host", b"host", b"HOST", b"Host", b"get", b"GET", b"user-agent", b"aB", b"ab", b"\xc1\xda", b"h", b"T", b"ABCDEabcdeABCDEabcde", b"abcdeABCDEabcdeABCDE"]
    flags = [False, True, True, True, True, False, True, True, False, True, True, False, True, False]
    payloads = [p.replace(b"\x01", b"Q") for p in nul_payloads(rng, 500, None, words)]
    arena = K.HostArena.from_payloads(payloads)
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, flags, whole=True)
    assert whole == MM.counts(MM.starts(payloads, pats, nocase=flags, whole=True))
    strlen = MM.counts(MM.starts(payloads, pats, whole=False, nocase=flags))
    assert whole != strlen and whole[0] != whole[1] and whole[1] == whole[2] == whole[3]
    reset(gm)
    gm.load_arena(arena)
    gm.set_patterns(pats, nocase=flags)
    for v in VARIANTS:
        select(gm, v)
        for opt, want in ((1, whole), (0, strlen)):
            gm.set_option(OPT_WHOLE_PAYLOAD, opt)
            assert gm.scan()[0].tolist() == want, (v[0], opt)
    reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. offsets   7. packets
# ------------------------------------------------------------------------------------------------
STREAMING = ((KERNEL_AUTO, 0), (KERNEL_PACKED, 0), (KERNEL_FLAT, 0), (KERNEL_AUTO, 1))


@pytest.mark.parametrize("uniform", [False, True])
def test_offsets(gm, oracle, uniform):
    rng = random.Random(61 + uniform)
    texts = [rand_text(rng, 300) for _ in range(10)]
    pats = cut_patterns(rng, texts, [2, 3, 5, 9, 17, 40], per=1) + [b"a", b"ab", b"E"]
    payloads = nul_payloads(rng, 400, 1500 if uniform else None, pats)
    arena = K.HostArena.from_payloads(payloads)
    st = MM.starts(payloads, pats, whole=True)
    model = sorted(MM.records(st))
    whole = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True)
    strlen = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats)
    assert whole != strlen and MM.counts(st) == whole
    behind = [(k, s, i) for k, s, i in model if 0 in payloads[k][:s]]
    assert behind
    reset(gm)
    gm.set_patterns(pats)
    gm.load_arena(arena)
    gm.set_option(OPT_ACCUMULATE, 1)
    gm.counts_reset()
    gm.scan()
    before = gm.counts_read().tolist()                        # the context's running total: untouched by the offsets calls
    for kernel, fused in STREAMING:
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        gm.set_option(OPT_WHOLE_PAYLOAD, 1)
        recs, found, counts = gm.scan_offsets(len(model) + 10)
        assert found == len(model) == sum(counts.tolist()) and counts.tolist() == whole, (kernel, fused)
        got = MM.triples(recs)
        assert got == model, (kernel, fused)
        assert set(behind) <= set(got)                        # records behind their payload's first 0x00
        recs, found, counts = gm.scan_offsets(7)              # a cap smaller than found: the full total all the same
        assert found == len(model) and len(recs) == 7 and counts.tolist() == whole and set(MM.triples(recs)) <= set(model)
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)
        recs, found, counts = gm.scan_offsets(len(model) + 10)
        assert counts.tolist() == strlen and MM.triples(recs) == sorted(MM.records(MM.starts(payloads, pats, whole=False))), (kernel, fused)
    assert gm.counts_read().tolist() == before
    reset(gm)


@pytest.mark.parametrize("uniform", [False, True])
def test_packets(gm, oracle, uniform):
    rng = random.Random(71 + uniform)
    texts = [rand_text(rng, 300) for _ in range(10)]
    pats = cut_patterns(rng, texts, [2, 4, 8, 16, 40], per=1) + [b"C", b"de"] + [rand_text(rng, 30)]
    pats.append(pats[1])                                      # a duplicate: identical rows
    payloads = nul_payloads(rng, 700, 1500 if uniform else None, pats[:-2])
    payloads[3] = b"\0" + pats[4] + rand_text(rng, 1500 - 1 - len(pats[4]) if uniform else 9)       # its only occurrences lie behind a 0x00
    arena = K.HostArena.from_payloads(payloads)
    n, P = len(payloads), len(pats)

    def expect(whole):
        st = MM.starts(payloads, pats, whole=whole)
        return MM.hits(st), MM.counts(st)

    hits_w, counts_w = expect(True)
    hits_s, counts_s = expect(False)
    assert counts_w == MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, whole=True) and counts_w != counts_s
    assert hits_w[4, 3] and not hits_s[:, 3].any() and (hits_w != hits_s).any()
    reset(gm)
    gm.set_patterns(pats)
    gm.load_arena(arena)
    gm.set_option(OPT_ACCUMULATE, 1)
    gm.counts_reset()
    gm.scan()
    before = gm.counts_read().tolist()
    for kernel, fused in STREAMING:
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        for opt, hits, counts in ((1, hits_w, counts_w), (0, hits_s, counts_s), (1, hits_w, counts_w)):
            gm.set_option(OPT_WHOLE_PAYLOAD, opt)
            r = gm.scan_packets(hits=True)
            assert np.array_equal(r["hits"], hits), (kernel, fused, opt)
            assert np.array_equal(r["any"], hits.any(axis=0)), (kernel, fused, opt)
            assert r["pkt_counts"].tolist() == hits.sum(axis=1).tolist() and r["counts"].tolist() == counts, (kernel, fused, opt)
            assert np.array_equal(r["hits"][1], r["hits"][-1])
    assert gm.counts_read().tolist() == before
    reset(gm)


# ------------------------------------------------------------------------------------------------
# 8. state
# ------------------------------------------------------------------------------------------------
def test_state_accumulate_and_bad_values(gm, oracle):
    import ctypes as C
    rng = random.Random(3)
    pats = [b"ab", b"AbC", b"c", b"\xc1", b"deABC"]
    batches = [nul_payloads(rng, 300, None, pats) for _ in range(3)]
    whole, strlen = [0] * len(pats), [0] * len(pats)
    for bt in batches:
        a = K.HostArena.from_payloads(bt)
        whole = [x + y for x, y in zip(whole, MM.oracle_counts_arena(oracle, a.bytes, a.off, a.len, pats, whole=True))]
        strlen = [x + y for x, y in zip(strlen, MM.oracle_counts_arena(oracle, a.bytes, a.off, a.len, pats))]
    assert whole != strlen
    reset(gm)
    gm.set_patterns(pats)
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    gm.set_option(OPT_ACCUMULATE, 1)
    gm.counts_reset()
    for bt in batches:
        gm.load_arena(K.HostArena.from_payloads(bt))
        gm.scan_enqueue()
    assert gm.counts_read().tolist() == whole
    gm.set_option(OPT_ACCUMULATE, 0)

    g = _lib.gpu_lib()
    last = K.HostArena.from_payloads(batches[-1])
    want_last = MM.oracle_counts_arena(oracle, last.bytes, last.off, last.len, pats, whole=True)
    for bad in (2, -1, 1 << 40):
        assert g.kmpgpu_set_option(gm._ctx, OPT_WHOLE_PAYLOAD, C.c_int64(bad)) == -2          # KMPGPU_EINVAL ...
        assert gm.scan()[0].tolist() == want_last                                    # ... and the option is unchanged
    gm.set_option(OPT_WHOLE_PAYLOAD, 0)
    assert g.kmpgpu_set_option(gm._ctx, OPT_WHOLE_PAYLOAD, C.c_int64(2)) == -2
    assert gm.scan()[0].tolist() == MM.oracle_counts_arena(oracle, last.bytes, last.off, last.len, pats)
    # a pattern that holds a 0x00 is refused in either mode, and the set in place stays
    u8p = C.POINTER(C.c_uint8)
    buf = np.frombuffer(b"ab\0d", dtype=np.uint8)
    ptrs = (u8p * 1)(buf.ctypes.data_as(u8p))
    lens = (C.c_uint32 * 1)(4)
    for opt in (1, 0):
        gm.set_option(OPT_WHOLE_PAYLOAD, opt)
        assert g.kmpgpu_set_patterns(gm._ctx, ptrs, lens, 1) == -2
        assert b"0x00" in g.kmpgpu_last_error()
    # the one-shot helper
    assert K.matcher.count_matches(pats, last, whole_payload=True).tolist() == want_last
    assert K.matcher.count_matches(pats, last).tolist() == MM.oracle_counts_arena(oracle, last.bytes, last.off, last.len, pats)
    assert K.matcher.OPT_WHOLE_PAYLOAD == 9
    reset(gm)


# ------------------------------------------------------------------------------------------------
# 9. fixtures
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", FIXTURE_KEYS)
def test_fixtures(gm, tokens, fixture_counts, whole_golden, key):
    pcap, mode = key.split(":")
    path = os.path.join(DATA, pcap)
    want, today = whole_golden[key]["counts"], fixture_counts["fixtures"][key]["counts"]
    reset(gm)
    gm.set_patterns(tokens)
    gm.load_arena(K.HostArena.from_pcap(path, mode))
    for v in (VARIANTS[0], VARIANTS[2], VARIANTS[3], VARIANTS[5]):
        select(gm, v)
        gm.set_option(OPT_WHOLE_PAYLOAD, 1)
        assert gm.scan()[0].tolist() == want, (key, v[0])
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)
        assert gm.scan()[0].tolist() == today, (key, v[0])
    reset(gm)
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    gm.load_pcap_frames(path, mode)                           # extraction on the device
    assert gm.scan()[0].tolist() == want, key
    gm.set_option(OPT_WHOLE_PAYLOAD, 0)
    assert gm.scan()[0].tolist() == today, key
    reset(gm)


def test_golden_sums(fixture_counts, whole_golden):
    sums = {k: (sum(fixture_counts["fixtures"][k]["counts"]), sum(whole_golden[k]["counts"])) for k in FIXTURE_KEYS}
    assert sums["udp.pcap:udp"] == (31, 39) and sums["udp_1000.pcap:udp"] == (927, 1006) and sums["big_udp.pcap:udp"] == (4129, 5752)
    assert sums["very_big_udp.pcap:udp"] == (0, 13863) and sums["tcp.pcap:tcp"] == (4, 4)


# ------------------------------------------------------------------------------------------------
# 10. the drop-in command lines: KMPGPU_WHOLE_PAYLOAD=1
# ------------------------------------------------------------------------------------------------
CLI_RUNS = [("serial", [], {}), ("openmp_data", ["2"], {}), ("openmp_task", ["2"], {"KMPGPU_DEVICE_EXTRACT": "0", "KMPGPU_BATCH_BYTES": "65536"}),
            ("openmp_task", ["1"], {"KMPGPU_DEVICE_EXTRACT": "1", "KMPGPU_BATCH_BYTES": "65536"}), ("serial", [], {"KMPGPU_DEVICE_EXTRACT": "1"}),
            ("serial", [], {"KMPGPU_RCCL": "1"})]


@pytest.mark.parametrize("key", ["udp_1000.pcap:udp", "very_big_udp.pcap:udp"])
@pytest.mark.parametrize("run", CLI_RUNS, ids=[f"{r[0]}-{i}" for i, r in enumerate(CLI_RUNS)])
def test_cli_whole_payload(tokens, fixture_counts, whole_golden, key, run):
    prog, extra, env_extra = run
    pcap, mode = key.split(":")
    want, today = whole_golden[key]["counts"], fixture_counts["fixtures"][key]["counts"]
    assert want != today
    r = run_cli(prog, pcap, extra=extra, env_extra=dict(env_extra, KMPGPU_WHOLE_PAYLOAD="1", KMPGPU_STATS="1"), mode=mode, scrub="KMPGPU_WHOLE_PAYLOAD")
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == K.format_report(tokens, want)
    assert "text rule: whole payloads" in r.stderr
    for unset in ({}, {"KMPGPU_WHOLE_PAYLOAD": "0"}):
        r = run_cli(prog, pcap, extra=extra, env_extra=dict(env_extra, **unset), mode=mode, scrub="KMPGPU_WHOLE_PAYLOAD")
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == K.format_report(tokens, today)


@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["3"])])
def test_cli_offsets_and_packets_files(tokens, tmp_path, prog, extra):
    host = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(host.payload(k)) for k in range(host.n_pkts)]
    for whole in (True, False):
        model = sorted(MM.records(MM.starts(payloads, tokens, whole=whole)))
        off, pk = tmp_path / f"offsets{whole}.csv", tmp_path / f"packets{whole}.csv"
        env = {"KMPGPU_OFFSETS_FILE": str(off), "KMPGPU_PACKETS_FILE": str(pk)}
        if whole:
            env["KMPGPU_WHOLE_PAYLOAD"] = "1"
        r = run_cli(prog, extra=extra, env_extra=env, scrub="KMPGPU_WHOLE_PAYLOAD")
        assert r.returncode == 0, r.stderr
        got = sorted(tuple(int(x) for x in line.split(",")) for line in off.read_text().splitlines() if line and line[0].isdigit())
        assert got == model, whole
        got = [tuple(int(x) for x in line.split(",")) for line in pk.read_text().splitlines() if line and line[0].isdigit()]
        assert got == sorted({(k, i) for k, _, i in model}), whole
    assert sorted(MM.records(MM.starts(payloads, tokens, whole=True))) != sorted(MM.records(MM.starts(payloads, tokens, whole=False)))


def test_mpi_dumping_whole_payload(tokens, fixture_counts, whole_golden):
    key = "big_udp.pcap:udp"
    for env_extra, want in (({"KMPGPU_WHOLE_PAYLOAD": "1"}, whole_golden[key]["counts"]), ({}, fixture_counts["fixtures"][key]["counts"])):
        env = {k: v for k, v in os.environ.items() if k != "KMPGPU_WHOLE_PAYLOAD"}
        env.update(KMPGPU_DIST_BACKEND="gloo", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_extra)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", "29581", "-m", "multithreading_string_matching_amd.mpi_dumping",
               os.path.join(DATA, "big_udp.pcap"), os.path.join(DATA, "strings.txt"), "udp"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout[r.stdout.index("Printing the number"):]
        assert strip_elapsed(out) == K.format_report(tokens, want)


# ------------------------------------------------------------------------------------------------
# 11. full size
# ------------------------------------------------------------------------------------------------
def _zipf_lengths(n, seed=4):
    rng = np.random.default_rng(seed)
    ranks = np.arange(1, 9000 - 64 + 2)
    p = 1.0 / ranks ** 1.1
    p /= p.sum()
    return (64 + rng.choice(len(ranks), size=n, p=p)).astype(np.uint32)


@pytest.mark.parametrize("shape", ["uniform_1500", "zipf_64_9000"])
def test_full_size_1m(gm, oracle, shape):
    """1 M synthetic payloads with 0x00 sprinkled at p = 1e-3 per byte and a planted needle: the flat / packed, general and fused kernels
    agree with each other on all payloads, and with remap + oracle on the first 100 000 payloads loaded alone (the cap bounds CPU time,
    not the coverage of the kernels' agreement)."""
    n = 1_000_000
    needle = b"NEEDLE_16B_PATRN"
    pats = [needle, b"NEEDLE", b"PATRN", b"th"]
    sp = K.SynthParams.make(seed=1234, needle=needle, plant_permille=100, nul_ppm=1000)
    if shape == "uniform_1500":
        off, ln, nbytes = K.arena_layout(None, 1500, n)
    else:
        lens = _zipf_lengths(n)
        lens[:5] = [9000, 8999, 64, 1024, 2048]
        off, ln, nbytes = K.arena_layout(lens, 0, n)
    d_arena = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    gm.set_stream(None)
    gm.synth_fill(d_arena, d_off, d_len, sp)
    gm.sync()
    reset(gm)
    gm.set_patterns(pats)
    gm.attach_arena(d_arena, d_off, d_len)
    results = {}
    for name, kernel, fused in (("auto", KERNEL_AUTO, 0), ("flat", KERNEL_FLAT, 0), ("packed", KERNEL_PACKED, 0), ("general", KERNEL_GENERAL, 0), ("fused", KERNEL_AUTO, 1)):
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        gm.set_option(OPT_WHOLE_PAYLOAD, 1)
        results[name] = gm.scan()[0].tolist()
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)
        results[name + "/strlen"] = gm.scan()[0].tolist()
    first, first_s = results["auto"], results["auto/strlen"]
    assert all(v == (first_s if k.endswith("/strlen") else first) for k, v in results.items()), results
    planted = K.synth_count_planted(sp, n, 1500 if shape == "uniform_1500" else 0, **({} if shape == "uniform_1500" else {"lens": lens}))
    assert 0 < first_s[0] < first[0] <= planted               # the needles behind a 0x00 count now; one hit by a 0x00 itself still does not
    ns = 100_000
    end = int(off[ns])
    host = d_arena[:end + 64].cpu().numpy()
    want = MM.oracle_counts_arena(oracle, host, off[:ns], ln[:ns], pats, whole=True, threads=8)
    assert want != MM.oracle_counts_arena(oracle, host, off[:ns], ln[:ns], pats, threads=8)
    gm.attach_arena(d_arena, d_off[:ns], d_len[:ns])
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    for name, kernel, fused in (("auto", KERNEL_AUTO, 0), ("packed", KERNEL_PACKED, 0), ("general", KERNEL_GENERAL, 0), ("fused", KERNEL_AUTO, 1)):
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        assert gm.scan()[0].tolist() == want, (shape, name)
    reset(gm)
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
