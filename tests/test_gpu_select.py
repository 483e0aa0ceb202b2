"""kmpgpu_load_selected (GpuMatcher.load_selected) on a real MI355X: the payloads a bitmap selects, compacted on the device into a
second context's arena.

The expectation is a numpy model, exact in every comparison: the selected indices are the set bits below n_src; the expected
index and arena are tests/prep_model.py's packed layout (gather_slots: every payload followed by 0x00 up to its slot's end) over
the source's payloads at those indices.  dst.arena_download() is compared over [0, end of the last slot) plus the 64 zero bytes
behind it, with index, arena_info and n_selected; counts on dst come from the CPU oracle over the selected payloads; hit rows,
rule rows and offsets from the host model of tests/match_model.py.

Where every kernel's second code path starts, read off the launchers of csrc/kmp_select.hip and csrc/kmp_prep.hip:

  row  code                                              second path starts at                                crossed by
  S1   kmp_select_lengths_kernel, a second bitmap word   > 64 payloads                                        test_sizes_and_densities[65 ...]
  S2   kmp_scan_local_kernel, a second tile              > 1 024 payloads (256 threads * 4 items)             test_sizes_and_densities[1025], test_at_scale
  S3   kmp_scan_totals_kernel, carries                   > 262 144 payloads (256 tiles per round)             test_at_scale (300 001)
  S4   kmp_select_lengths_kernel and                     > 262 144 payloads (KMP_GRID_CAP 1 024    test_at_scale
       kmp_select_index_kernel: grid-stride                * 256 threads)
  S5   kmp_select_copy_kernel, r += waves                > 4 096 runs (KMP_GRID_CAP 1 024 * 4       test_at_scale[all, random_0.9, words, alternating]:
                                                           waves); a run is 64 payloads at these sizes           > 262 144 selected payloads
  S6   kmp_select_copy_kernel, run length                64 payloads per run while the average slot is        test_sizes_and_densities (1 500- and 9 000-byte
                                                           <= 256 bytes, halved down to 1 from there on         payloads among 16-byte ones), test_dst_state_* (uniform
                                                           (KMP_RUN_BYTES 16 384)                        1 500: runs of 8), test_long_payloads (runs of 1)
  S7   kmp_select_copy_kernel, a run of more than        a lane's second step: runs of > 4 KiB                every test with payloads of 100 bytes and more
       4 * 64 units
  S8   source offsets as 64-bit values                   > 4 GiB                                              test_source_past_4_gib
  S9   destination offsets as 64-bit values              > 4 GiB                                              tests/test_gpu_high_destinations.py::test_selected_past_2_32

No test provokes a fault: every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_select.py -m gpu
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

from gpu_support import reset, run_cli, strip_elapsed  # noqa: E402  (torch first)

import torch  # noqa: E402

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
import prep_model as PM  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    OPT_NONTEMPORAL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher, device_count, select_words, selected_indices)
from test_gpu_windows import check_all, make_payloads, random_rules, random_windows, sub  # noqa: E402

EINVAL, ESTATE = -2, -3
LENGTHS = [0, 1, 15, 16, 17, 48, 1500, 9000]
SIZES = [1, 63, 64, 65, 1023, 1024, 1025]
N_SCALE = 300_001
INDEX_ITEMS = 1024 * 256         # one grid-stride round of kmp_select_lengths_kernel / kmp_select_index_kernel; one round of kmp_scan_totals_kernel
COPY_RUNS = 1024 * 4             # runs one round of kmp_select_copy_kernel covers
assert N_SCALE > INDEX_ITEMS and N_SCALE > 64 * COPY_RUNS
DENSITIES = ["none", "all", "first", "last", "alternating", "words", "random_0.1", "random_0.9"]
PATS = [b"ab", b"abcab", b"b", b"cabcabcabcab", b"ca"]
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


@pytest.fixture(scope="module")
def src():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def dst():
    m = GpuMatcher(0)
    yield m
    m.close()


def density(name, n, seed=0):
    rng = np.random.default_rng(seed)
    sel = np.zeros(n, dtype=bool)
    if name == "all":
        sel[:] = True
    elif name == "first":
        sel[0] = True
    elif name == "last":
        sel[-1] = True
    elif name == "alternating":
        sel[::2] = True
    elif name == "words":                       # whole bitmap words of ones and of zeros, a zero word first
        sel[:] = (np.arange(n) // 64) % 3 == 1
    elif name.startswith("random_"):
        sel[:] = rng.random(n) < float(name[7:])
    else:
        assert name == "none"
    return sel


def text_arena(ln, seed, nul_permille=3):
    """A packed arena of payloads of the given lengths over {a, b, c} with a few 0x00 bytes, padding clean."""
    rng = np.random.default_rng(seed)
    ln = np.asarray(ln, dtype=np.uint32)
    off = PM.packed_offsets(ln)
    end = int(off[-1] + PM.slot_bytes(ln)[-1]) if len(ln) else 0
    arena = rng.integers(ord("a"), ord("c") + 1, end + 64).astype(np.uint8)
    arena[rng.random(end + 64) < nul_permille / 1000.0] = 0
    arena = PM.clean_padding(arena, off, ln)
    arena[end:] = 0
    return arena, off, ln


def expected(arena, off, ln, idx):
    """(pkt_off, pkt_len, arena up to the last slot's end) of the selection idx of a source"""
    idx = np.asarray(idx, dtype=np.int64)
    sl = np.asarray(ln)[idx].astype(np.uint32)
    new_off, packed = PM.gather_slots(arena, np.asarray(off)[idx], sl)
    return new_off, sl, packed


def first_diff(a, b):
    d = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return None if len(d) == 0 else (int(d[0]), len(d))


def check_arena(dst, want_off, want_len, want_arena):
    n = len(want_len)
    assert dst.arena_info() == (n, int(np.asarray(want_len).sum(dtype=np.uint64)))
    a2, off2, ln2 = dst.arena_download()
    if n == 0:
        assert len(off2) == len(ln2) == 0
        return
    assert len(ln2) == n and first_diff(ln2, want_len) is None
    assert first_diff(off2, want_off) is None
    assert len(a2) == len(want_arena) + 64 and first_diff(a2[:len(want_arena)], want_arena) is None        # payload bytes AND zero padding
    assert not a2[len(want_arena):].any()


def select_and_check(dst, src, source, sel, oracle=None, pats=None, device=False):
    """source = (arena, off, len) of what src holds, on the host; sel: bool[n_src]"""
    arena, off, ln = source
    words = select_words(sel, len(ln))
    arg = torch.from_numpy(words.view(np.int64)).cuda() if device else sel
    idx = dst.load_selected(src, arg)
    assert idx.tolist() == np.flatnonzero(sel).tolist()
    want_off, want_len, want_arena = expected(arena, off, ln, idx)
    check_arena(dst, want_off, want_len, want_arena)
    t = dst.last_timing()
    if len(idx):
        assert t.launches == 5 and t.kernel_ms > 0
    assert (t.h2d_bytes, t.h2d_ms > 0) == ((0, False) if device else (8 * len(words), True))
    if oracle is not None:
        want = oracle.count(want_arena, want_off, want_len, pats, threads=8)[0] if len(idx) else np.zeros(len(pats), np.uint64)
        assert dst.scan()[0].tolist() == want.tolist()
    return idx, (want_arena, want_off, want_len)


# ------------------------------------------------------------------------------------------------
# 1. sizes x densities, a packed source (S1, S2, S6, S7)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_densities(src, dst, oracle, n):
    rng = np.random.default_rng(n)
    ln = rng.choice(LENGTHS, n)
    if n >= 63:
        ln[:len(LENGTHS)] = LENGTHS                            # every length is there, the empty payload first
    source = text_arena(ln, seed=n)
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.load_arena(*source)
        for name in DENSITIES:
            for device in (False, True):
                sel = density(name, n, seed=n)
                idx, _ = select_and_check(dst, src, source, sel, oracle, PATS, device=device)
                assert len(idx) == int(sel.sum())
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 2. past every grid cap and one round of the totals kernel (S3, S4, S5)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale_source():
    rng = np.random.default_rng(300001)
    return text_arena(rng.integers(0, 49, N_SCALE), seed=2)


@pytest.mark.parametrize("name", DENSITIES)
def test_at_scale(src, dst, oracle, scale_source, name):
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        if src.arena_info()[0] != N_SCALE:
            src.load_arena(*scale_source)
        sel = density(name, N_SCALE, seed=7)
        idx, _ = select_and_check(dst, src, scale_source, sel, oracle, PATS, device=(name == "words"))
        if name in ("all", "random_0.9"):
            assert len(idx) > 64 * COPY_RUNS
        if name != "none":
            assert len(idx) > 0 and (name in ("first", "last") or len(idx) > 1024)
    finally:
        reset(src, dst)


def test_long_payloads(src, dst, oracle):
    """payloads of 20 000 to 70 000 bytes: a run is one payload, a wavefront walks it in steps of 4 KiB"""
    rng = np.random.default_rng(9)
    source = text_arena(rng.integers(20_000, 70_001, 200), seed=9, nul_permille=0)
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.load_arena(*source)
        for name in ("random_0.9", "alternating", "last"):
            select_and_check(dst, src, source, density(name, 200, seed=1), oracle, PATS)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


def test_selection_of_empty_payloads_only(src, dst, oracle):
    rng = np.random.default_rng(4)
    ln = rng.choice([0, 0, 5, 40], 3000)
    source = text_arena(ln, seed=4)
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.load_arena(*source)
        sel = (ln == 0) & (rng.random(3000) < 0.7)
        idx, (arena, off, sl) = select_and_check(dst, src, source, sel, oracle, PATS)
        assert len(idx) > 600 and int(sl.max()) == 0 and not arena.any() and len(arena) == 16 * len(idx)
        res = dst.scan_packets(hits=True)
        assert not res["hits"].any() and res["counts"].tolist() == [0] * len(PATS)
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 3. every kind of source
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gaps_repacked", "gaps_in_place"])
def test_source_with_gaps_and_shuffled_slots(src, dst, oracle, kind):
    n = 5000
    arena, off, ln = PM.shuffled_arena(n, seed=12)
    pats = [b"ab", b"abcab", b"b", b"cabcab"]
    try:
        reset(src, dst)
        src.set_patterns(pats); dst.set_patterns(pats)
        src.set_option(OPT_REPACK, 1 if kind == "gaps_repacked" else 0)
        src.load_arena(arena, off, ln)
        before = src.arena_download()
        if kind == "gaps_in_place":
            assert first_diff(before[1], off) is None                        # not packed: the index is followed as it is
        for name in ("random_0.1", "random_0.9", "alternating", "all"):
            sel = density(name, n, seed=3)
            # the payloads are the caller's whatever src made of their slots
            select_and_check(dst, src, (arena, off, ln), sel, oracle, pats)
        after = src.arena_download()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    finally:
        reset(src, dst)


def test_borrowed_source_with_dirty_padding(src, dst, oracle):
    """attach_arena of a torch buffer whose slot padding is 0xAA: dst's padding is zero, the source's bytes stay"""
    rng = np.random.default_rng(13)
    n = 4000
    arena, off, ln = text_arena(rng.choice(LENGTHS[:6] + [100, 333], n), seed=13)
    end = int(off[-1] + PM.slot_bytes(ln)[-1])
    dirty = np.full(len(arena), 0xAA, dtype=np.uint8)
    keep = PM.clean_padding(np.ones(len(arena), np.uint8), off, ln).astype(bool)
    keep[end:] = False
    dirty[keep] = arena[keep]
    assert (dirty[:end] == 0xAA).sum() > n
    d = (torch.from_numpy(dirty).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.attach_arena(*d)
        for name in ("random_0.9", "alternating", "all", "last"):
            for device in (False, True):
                select_and_check(dst, src, (arena, off, ln), density(name, n, seed=5), oracle, PATS, device=device)
        assert np.array_equal(d[0].cpu().numpy(), dirty) and np.array_equal(d[1].cpu().numpy(), off.astype(np.int64))
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


def test_source_extracted_from_frames(src, dst, oracle, tokens):
    path = os.path.join(DATA, "udp_1000.pcap")
    host = K.HostArena.from_pcap(path, "udp")
    source = (np.array(host.bytes), np.array(host.off), np.array(host.len))
    try:
        reset(src, dst)
        src.set_patterns(tokens); dst.set_patterns(tokens)
        n_pay, _ = src.load_pcap_frames(path, "udp")
        assert n_pay == host.n_pkts
        for name in ("random_0.1", "random_0.9", "words"):
            select_and_check(dst, src, source, density(name, n_pay, seed=6), oracle, tokens)
    finally:
        reset(src, dst)


def test_source_past_4_gib(src, dst, oracle):
    """A borrowed buffer a little over 4 GiB with a few hundred payloads at its end: source offsets as 64-bit values"""
    rng = np.random.default_rng(14)
    n = 300
    arena, off, ln = text_arena(rng.choice([0, 1, 17, 48, 1500, 9000], n), seed=14)
    end = int(off[-1] + PM.slot_bytes(ln)[-1])
    base = (1 << 32) + 4096
    d_big = torch.zeros(base + end + 64, dtype=torch.uint8, device="cuda")
    d_big[base:base + end] = torch.from_numpy(arena[:end]).cuda()
    d_off = torch.from_numpy((off + np.uint64(base)).astype(np.int64)).cuda()
    d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.attach_arena(d_big, d_off, d_len)
        for name in ("random_0.9", "all", "first", "last"):
            select_and_check(dst, src, (arena, off, ln), density(name, n, seed=8), oracle, PATS)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)
        del d_big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 4. the bitmap
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_bits_above_n_src_are_ignored(src, dst, oracle, n):
    rng = np.random.default_rng(40 + n)
    source = text_arena(rng.choice(LENGTHS[:7], n), seed=40 + n)
    W = (n + 63) // 64
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.load_arena(*source)
        sel = density("random_0.9", n, seed=1)
        words = select_words(sel, n)
        words[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))           # every bit at n and above
        ones = np.full(W, np.uint64((1 << 64) - 1))
        for w, want_sel in ((words, sel), (ones, np.ones(n, bool))):
            got = []
            for arg in (w, torch.from_numpy(w.view(np.int64)).cuda()):
                idx = dst.load_selected(src, arg)
                assert idx.tolist() == np.flatnonzero(want_sel).tolist()
                check_arena(dst, *expected(*source, idx))
                got.append([x.copy() for x in dst.arena_download()] + [dst.scan()[0]])
            assert all(np.array_equal(x, y) for x, y in zip(*got))                # host and device bitmap: identical results
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 5. dst: buffers reused, derived state rebuilt; src: untouched
# ------------------------------------------------------------------------------------------------
def test_large_then_small_selection_into_one_context(src, dst, oracle):
    rng = random.Random("reuse")
    plant = [b"abca", b"dA", b"bbbbb", b"cdcdcdcdcdcdcdcdcd"]
    payloads = make_payloads(rng, "mixed", plant, n=400)
    pats = plant + [sub(rng, payloads, m) for m in (1, 7)]
    rules = [([0], [1]), ([2, 4], []), ([], [5])]
    try:
        reset(src, dst)
        src.set_patterns(pats); dst.set_patterns(pats); dst.set_rules(rules)
        src.load_arena(K.HostArena.from_payloads(payloads))
        for sel in (np.ones(400, bool), np.arange(400) % 57 == 3, np.zeros(400, bool), np.arange(400) >= 395):
            idx = dst.load_selected(src, sel)
            mine = [payloads[int(k)] for k in idx]
            if not mine:
                assert dst.arena_info() == (0, 0) and dst.scan()[0].tolist() == [0] * len(pats)
                continue
            check_all(dst, oracle, mine, pats, None, rules)
    finally:
        reset(src, dst)


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_dst_state_nocase_rules_windows(src, dst, oracle, kind):
    """patterns with mixed nocase flags, rules and windows set on dst BEFORE the call: fold, bitmap and plans are rebuilt for
    the new arena, on each kernel family (check_all: auto / fused, flat -- taken on the uniform selection --, packed)"""
    rng = random.Random(f"select-{kind}")
    plant = [b"ABab", b"aBc", b"dAbCa", bytes(rng.choice(b"abcdAB") for _ in range(17))]
    payloads = make_payloads(rng, kind, plant, n=300)
    pats = plant + [sub(rng, payloads, m) for m in (1, 2, 6, 16)] + [b"abab", b"ABAB"]
    nocase = [True, False, True, True, True, False, True, False, True, False]
    windows = random_windows(rng, len(pats))
    windows[0], windows[1] = (0, 17), (0, None)
    rules = random_rules(rng, len(pats))
    try:
        reset(src, dst)
        src.set_patterns(pats[:2])
        dst.set_patterns(pats, nocase=nocase); dst.set_windows(windows); dst.set_rules(rules)
        dst.load_arena(K.HostArena.from_payloads(payloads[:40]))                   # an arena, a fold and plans of its own first
        assert dst.scan()[0].tolist() == MM.oracle_counts(oracle, payloads[:40], pats, nocase)
        src.load_arena(K.HostArena.from_payloads(payloads))
        for name in ("random_0.9", "alternating"):
            idx = dst.load_selected(src, density(name, len(payloads), seed=2))
            mine = [payloads[int(k)] for k in idx]
            assert dst.windows == windows and dst.rules == rules
            recs, hits, _ = check_all(dst, oracle, mine, pats, windows, rules, nocase=nocase)
            assert hits.any()
    finally:
        reset(src, dst)


def test_dst_state_whole_payload(src, dst, oracle):
    rng = random.Random("select-whole")
    pats = [b"XY", b"XYZW_", b"Z", b"XYZW_longer_than_16b", b"XY"]
    windows = [(20, 60), (0, 1100), (1000, None), (16, 1030), (0, 10)]
    rules = [([0], [4]), ([1, 2], []), ([], [3])]
    payloads = []
    for k in range(240):
        L = 1500 if k < 100 else rng.randrange(80, 2100)
        b = bytearray(rng.choice(b"abcd") for _ in range(L))
        for p, (a, _) in zip(pats, windows):
            s = a + rng.randrange(50)
            if s + len(p) <= L and rng.random() < 0.6:
                b[s:s + len(p)] = p
        if k % 3:
            b[rng.choice([5, 15, 16, 30, 999, 1023, 1024]) % L] = 0
        payloads.append(bytes(b))
    try:
        reset(src, dst)
        src.set_patterns(pats)
        dst.set_patterns(pats); dst.set_windows(windows); dst.set_rules(rules)
        dst.set_option(OPT_WHOLE_PAYLOAD, 1)
        src.load_arena(K.HostArena.from_payloads(payloads))
        idx = dst.load_selected(src, density("random_0.9", len(payloads), seed=3))
        mine = [payloads[int(k)] for k in idx]
        seen = {}
        for whole in (1, 0):
            dst.set_option(OPT_WHOLE_PAYLOAD, whole)
            seen[whole] = check_all(dst, oracle, mine, pats, windows, rules, whole=bool(whole))[0]
        assert seen[0] < seen[1]
        # the first 100 alone: a uniform selection of 1500-byte payloads
        dst.set_option(OPT_WHOLE_PAYLOAD, 1)
        idx = dst.load_selected(src, np.arange(len(payloads)) < 100)
        check_all(dst, oracle, payloads[:100], pats, windows, rules, whole=True)
    finally:
        reset(src, dst)


def test_default_cache_policy(src, dst, oracle):
    """OPT_NONTEMPORAL = 0 on dst: the other instantiation of the copy kernel"""
    rng = np.random.default_rng(15)
    source = text_arena(rng.choice(LENGTHS, 2000), seed=15)
    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        dst.set_option(OPT_NONTEMPORAL, 0)
        src.load_arena(*source)
        select_and_check(dst, src, source, density("random_0.9", 2000, seed=1), oracle, PATS)
    finally:
        reset(src, dst)


def test_src_is_untouched(src, dst, oracle):
    rng = random.Random("untouched")
    plant = [b"abca", b"dA", b"bbbbb"]
    payloads = make_payloads(rng, "mixed", plant, n=300)
    try:
        reset(src, dst)
        src.set_patterns(plant, nocase=[False, True, False]); dst.set_patterns(plant[:1])
        src.load_arena(K.HostArena.from_payloads(payloads))

        def snapshot():
            res = src.scan_packets(hits=True)
            return [x.copy() for x in src.arena_download()] + [src.scan()[0], res["hits"], res["any"], res["pkt_counts"], res["counts"]]

        before = snapshot()
        for name in ("random_0.9", "none", "all"):
            dst.load_selected(src, density(name, 300, seed=4))
            after = snapshot()
            assert all(np.array_equal(x, y) for x, y in zip(before, after)), name
        assert src.arena_info()[0] == 300
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 6. the cascade
# ------------------------------------------------------------------------------------------------
def test_cascade_on_a_capture(src, dst, oracle, tokens):
    """stage 1: one token, its any[] selects (the device words of a torch tensor, as a pipeline would hand them on); stage 2: the
    97 tokens over the subset.  Rows mapped back through the returned indices are the rows of a full pass restricted to them."""
    host = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(host.payload(k)) for k in range(host.n_pkts)]
    free_hits = MM.hits(MM.starts(payloads, tokens))
    per = free_hits.sum(axis=1)
    first = int(np.argmin(np.where((per >= 20) & (per < len(payloads)), per, 1 << 30)))       # a token in some payloads, not in all
    try:
        reset(src, dst)
        src.set_patterns([tokens[first]]); dst.set_patterns(tokens)
        src.load_arena(host)
        any1 = src.scan_packets()["any"]
        assert any1.tolist() == free_hits[first].tolist() and 20 <= any1.sum() < len(payloads)
        idx = dst.load_selected(src, torch.from_numpy(select_words(any1, len(payloads)).view(np.int64)).cuda())
        assert idx.tolist() == np.flatnonzero(any1).tolist()
        mine = [payloads[int(k)] for k in idx]
        res = dst.scan_packets(hits=True)
        assert res["counts"].tolist() == [int(x) for x in oracle.count_payloads(mine, tokens)]
        src.set_patterns(tokens)
        full = src.scan_packets(hits=True)
        assert np.array_equal(full["hits"], free_hits)
        assert np.array_equal(res["hits"], full["hits"][:, idx.astype(np.int64)])
        assert res["hits"][first].all()
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 7. life cycle and errors, through the raw ABI
# ------------------------------------------------------------------------------------------------
def test_life_cycle_and_errors(src, dst, oracle):
    g = _lib.gpu_lib()
    rng = np.random.default_rng(16)
    source = text_arena(rng.choice(LENGTHS[:7], 500), seed=16)
    kept = text_arena(rng.choice(LENGTHS[:7], 77), seed=17)
    want_kept = oracle.count(*kept, PATS, threads=8)[0].tolist()
    words = np.full(8, np.uint64((1 << 64) - 1))
    n_out = C.c_uint64(12345)

    def call(d, s, sel, on_device=0):
        return g.kmpgpu_load_selected(d, s, sel, on_device, C.byref(n_out))

    def dst_keeps_its_arena(rc, code):
        assert rc == code, (rc, code)
        assert b"kmpgpu_load_selected" in g.kmpgpu_last_error()
        assert n_out.value == 0
        assert dst.arena_info() == (77, int(kept[2].sum()))
        assert dst.scan()[0].tolist() == want_kept

    try:
        reset(src, dst)
        src.set_patterns(PATS); dst.set_patterns(PATS)
        src.load_arena(*source)
        dst.load_arena(*kept)
        p = words.ctypes.data
        dst_keeps_its_arena(call(dst._ctx, dst._ctx, p), EINVAL)
        dst_keeps_its_arena(call(None, src._ctx, p), EINVAL)
        dst_keeps_its_arena(call(dst._ctx, None, p), EINVAL)
        dst_keeps_its_arena(call(dst._ctx, src._ctx, None), EINVAL)
        dst_keeps_its_arena(call(dst._ctx, src._ctx, p, 2), EINVAL)
        dst_keeps_its_arena(call(dst._ctx, src._ctx, p, -1), EINVAL)
        # between kmpgpu_load_frames_begin and _finish, on either side
        path = os.path.join(DATA, "udp_1000.pcap")
        fr = _lib.Frames()
        err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
        assert _lib.host_lib().kmp_frames_from_pcap(path.encode(), None, None, C.byref(fr), err) == 0
        try:
            with GpuMatcher(0) as other:
                other.set_patterns(PATS)
                assert g.kmpgpu_load_frames_begin(other._ctx, fr.bytes, fr.nbytes, fr.off, fr.caplen, fr.n, 0) == 0
                dst_keeps_its_arena(call(dst._ctx, other._ctx, p), ESTATE)                      # src is loading
                rc = call(other._ctx, src._ctx, p)                                             # dst is loading
                assert rc == ESTATE and b"kmpgpu_load_selected" in g.kmpgpu_last_error()
                n_pay = C.c_uint64()
                assert g.kmpgpu_load_frames_finish(other._ctx, C.byref(n_pay)) == 0 and n_pay.value > 64
                W = (n_pay.value + 63) // 64
                assert call(dst._ctx, other._ctx, np.full(W, np.uint64(1)).ctypes.data) == 0 and n_out.value == W
                dst.load_arena(*kept)
        finally:
            _lib.host_lib().kmp_frames_free(C.byref(fr))
        # src without an arena: nothing selected, dst empty, select may be NULL
        src.load_arena(*EMPTY)
        n_out.value = 12345
        assert call(dst._ctx, src._ctx, None) == 0 and n_out.value == 0
        assert dst.arena_info() == (0, 0) and dst.scan()[0].tolist() == [0] * len(PATS)
        assert dst.scan_packets(hits=True)["hits"].shape == (len(PATS), 0)
        # a selection after the empty one, and its timing
        src.load_arena(*source)
        select_and_check(dst, src, source, density("random_0.1", 500, seed=9), oracle, PATS)
        assert dst.last_timing().launches > 0
    finally:
        reset(src, dst)


def test_two_devices_are_refused(src):
    if device_count() < 2:
        pytest.skip("one device")
    g = _lib.gpu_lib()
    with GpuMatcher(1) as far:
        far.set_patterns(PATS)
        source = text_arena([5, 40, 0], seed=18)
        src.load_arena(*source)
        words = np.full(1, np.uint64(7))
        n_out = C.c_uint64()
        assert g.kmpgpu_load_selected(far._ctx, src._ctx, words.ctypes.data, 0, C.byref(n_out)) == EINVAL
        assert b"kmpgpu_load_selected" in g.kmpgpu_last_error() and far.arena_info() == (0, 0)


# ------------------------------------------------------------------------------------------------
# 8. the command lines: KMPGPU_EXPORT_FILE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"]), ("openmp_data", ["2"])])
def test_cli_export_file(tokens, tmp_path, prog, extra):
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(arena.payload(k)) for k in range(arena.n_pkts)]
    free_hits = MM.hits(MM.starts(payloads, tokens))
    busy = [int(i) for i in np.argsort(-free_hits.sum(axis=1))[:6]]
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        golden = f.read()
    plain = run_cli(prog, extra=extra, env_extra={})
    assert plain.returncode == 0 and strip_elapsed(plain.stdout) == golden

    def exported(env):
        out = tmp_path / "export.pcap"
        if out.exists():
            out.unlink()
        r = run_cli(prog, extra=extra, env_extra=dict(env, KMPGPU_EXPORT_FILE=str(out)))
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == golden                                         # stdout as without the variable
        back = K.HostArena.from_pcap(str(out), "udp")
        return [bytes(back.payload(k)) for k in range(back.n_pkts)]

    # the payloads that hold at least one pattern
    want = [payloads[int(k)] for k in np.flatnonzero(free_hits.any(axis=0))]
    assert 0 < len(want)
    assert exported({}) == want
    # with a rules file (and no alerts file): the payloads at least one rule matches
    rules = [([busy[4]], [busy[5]]), ([busy[5], busy[1]], [busy[4]])]
    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([str(i) for i in pos] + [f"!{i}" for i in neg]) + "\n" for pos, neg in rules))
    rows = MM.rule_rows(free_hits, rules)
    want = [payloads[int(k)] for k in np.flatnonzero(rows.any(axis=0))]
    assert 0 < len(want) < int(free_hits.any(axis=0).sum())
    assert exported({"KMPGPU_RULES_FILE": str(rf)}) == want
    # with a windows file and no other output file: the windows decide what a hit is
    windows = [(0, None)] * len(tokens)
    text = ""
    for i in range(len(tokens)):                       # one token anywhere, one only at the payload's head, the others behind every payload's end
        windows[i] = (0, None) if i == busy[5] else (0, 3) if i == busy[4] else (4000, 5000)
        text += f"{i} {windows[i][0]} {'*' if windows[i][1] is None else windows[i][1]}\n"
    wf = tmp_path / "windows.txt"
    wf.write_text(text)
    hits = MM.hits(MM.starts(payloads, tokens, windows))
    want = [payloads[int(k)] for k in np.flatnonzero(hits.any(axis=0))]
    assert 0 < len(want) < int(free_hits.any(axis=0).sum())
    assert exported({"KMPGPU_WINDOWS_FILE": str(wf)}) == want
