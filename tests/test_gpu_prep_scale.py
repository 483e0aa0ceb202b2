"""The kernels that BUILD the arena (csrc/kmp_prep.hip, kmp_slot_end_kernel of kmp_fold.hip) past their tile and grid sizes,
against the numpy model of tests/prep_model.py (itself held to the host library and the oracle by tests/test_prep_model.py).

The frames of kmpgpu_load_frames may repeat, so a library of a few hundred distinct frames and an index of millions of entries
into it gives inputs of any size with a tiny upload; the expected arena follows from numpy, and the tags ``<K00042>`` at the
head of the library's payloads pin every payload of the device arena to its source (count(tag k) == accepted entries of kind k).

Where every kernel's second code path starts, read off the launchers (KMP_BLOCK_THREADS 256, KMP_BLOCK_WAVES 4, KMP_SCAN_ITEMS 4):

  row  code                                            second path starts at                               crossed by
  R1   kmp_scan_local_kernel, a second tile            > 1 024 items (tile = 256 threads * 4 items)         test_extraction_at_threshold_edges, test_repack_at_scale
  R2   kmp_scan_totals_kernel, carries cb / cc         > 262 144 items (256 tiles per round of the loop)    test_extraction_at_threshold_edges[262145...], test_extraction_sequence_shapes[empty_rounds],
                                                                                                            test_repack_at_scale[262145, 1300003]
  R3   kmp_gather_kernel, k += nw                      > 32 768 payloads (grid cap 8 192 blocks * 4 waves)  test_extraction_at_threshold_edges[>= 262143], test_repack_at_scale[262145, 1300003]
  R4   kmp_extract_kernel, kmp_scatter_index_kernel,   > 1 048 576 items (grid cap 4 096 blocks * 256)      test_extraction_at_threshold_edges[1048577, 2500123], test_repack_at_scale[1300003]
       kmp_repack_index_kernel: grid-stride
  R5   kmp_check_padding_kernel, fix and no fix        > 2 097 152 payloads (grid cap 8 192 * 256)          test_padding_at_scale
  R6   kmp_effective_bytes_kernel, k += nw             > 32 768 payloads (8 192 * 4 waves)                  test_effective_bytes_at_scale, the extraction and repack tests
  R7   kmp_validate_index_kernel, flags in a later     > 524 288 payloads (grid cap 2 048 * 256)            test_layout_check_on_the_device, test_uniform_index_with_one_odd_length
       grid-stride round
  R8   kmp_slot_end_kernel (kmp_fold.hip)              > 262 144 payloads (grid cap 1 024 * 256)            test_repack_at_scale[1300003] (borrowed, in place, nocase)
  R9   file + frame_off[f], src_off[k], pkt_off[k]     > 4 GiB                                              test_arena_past_4_gib, test_source_past_4_gib
       as 64-bit values
  R10  kmpgpu_attach_arena of a borrowed, non-packed   any size                                             test_repack_at_scale (route "attach")
       arena (device-side check -> repack)
  R11  the arena buffers and the install path that    buffers grow, are reused, are given back            test_one_context_through_every_loader
       every loader shares (csrc/kmpgpu.hip)

Checked to bite: with each of these memory-safe changes made to a scratch build, tests here failed while the rest of the GPU
suite passed -- the carry cb, or cc, of kmp_scan_totals_kernel not applied to the tiles' prefixes (totals kept; R2: the
threshold-edge tests from 262 145 on, empty_rounds, both 4 GiB tests; cb also the repack tests); kmp_gather_kernel stopping
after a wavefront's first payload (R3: every extraction and repack test past 32 768 payloads); kmp_check_padding_kernel after
a thread's first payload (R5: both test_padding_at_scale); kmp_effective_bytes_kernel likewise (R6: test_effective_bytes_at_scale
and the extraction / repack tests); kmp_extract_kernel rejecting every frame of a later grid-stride round (R4: 1048577-udp,
2500123, last_only, empty_rounds, all_empty); kmp_validate_index_kernel dropping the flags of later rounds (R7:
test_layout_check_on_the_device[700001] and [999999]).

Every negative case is one the library refuses in its check kernel, which reads the index only; the device buffers of those
cases are large enough for the bad entry as well.

Run on a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import gm, lib, load_frames as _load_frames, reset  # noqa: E402,F401  (torch first; gm, lib: fixtures)

import torch  # noqa: E402

import prep_model as PM  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd._lib import KmpGpuError  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_GENERAL, KERNEL_PACKED, MODE_FILTER, OPT_FUSED, OPT_KERNEL, OPT_MODE, OPT_REPACK, GpuMatcher)

KERNEL_FUSED = 100          # test-only alias: auto kernel selection + the fused multi-pattern pass
TILE = 256 * 4              # KMP_SCAN_TILE
ROUND = 256 * TILE          # one round of kmp_scan_totals_kernel
GATHER_WAVES = 8192 * 4     # payloads one round of kmp_gather_kernel / kmp_effective_bytes_kernel covers
GRID_ITEMS = 4096 * 256     # one grid-stride round of the extract / scatter / repack-index kernels
PAD_ITEMS = 8192 * 256      # ... of kmp_check_padding_kernel
VALIDATE_ITEMS = 2048 * 256  # ... of kmp_validate_index_kernel
SLOT_END_ITEMS = 1024 * 256  # ... of kmp_slot_end_kernel
N_BIG = 2_500_123           # ten rounds of the totals kernel, the last one partial; not a multiple of 1 024
assert N_BIG % TILE and (N_BIG + ROUND - 1) // ROUND == 10 and PM.ROUND_ITEMS == ROUND


def _scan(gm, kernel):
    gm.set_option(OPT_MODE, MODE_FILTER)
    gm.set_option(OPT_KERNEL, KERNEL_AUTO if kernel == KERNEL_FUSED else kernel)
    gm.set_option(OPT_FUSED, 1 if kernel == KERNEL_FUSED else 2 if kernel == KERNEL_AUTO else 0)
    return gm.scan()[0]


def _first_diff(a, b):
    d = np.flatnonzero(a != b)
    return None if len(d) == 0 else (int(d[0]), len(d))


def _check_extraction(gm, lib, proto, kind, two_steps=False, packed_tags=True):
    """Load the frame sequence `kind` and compare everything the device made of it with the model."""
    poff, plen, payloads = lib.rule[proto]
    n_pay = _load_frames(gm, lib.blob, lib.boff[kind], lib.cap[kind], proto, two_steps)
    acc, off, ln, arena = PM.extraction_arena(lib.blob, lib.boff, poff, plen, kind)
    assert n_pay == len(acc)
    assert gm.arena_info() == (len(acc), int(ln.sum(dtype=np.uint64)))
    if len(acc) == 0:
        assert _scan(gm, KERNEL_AUTO).tolist() == [0] * lib.K
        assert gm.effective_bytes() == 0
        return acc
    a2, off2, ln2 = gm.arena_download()
    assert len(ln2) == len(ln) and _first_diff(ln2, ln) is None
    assert _first_diff(off2, off) is None
    assert len(a2) == len(arena) + 64 and _first_diff(a2[:len(arena)], arena) is None       # payload bytes AND zero padding
    assert not a2[len(arena):].any()
    assert gm.effective_bytes() == PM.effective_bytes(arena, off, ln)
    want = PM.tag_counts(payloads, acc, lib.K)
    assert _scan(gm, KERNEL_FUSED).tolist() == want.tolist()
    if packed_tags:
        assert _scan(gm, KERNEL_PACKED).tolist() == want.tolist()
    own = PM.own_tag_kinds(payloads)
    assert want[own].tolist() == np.bincount(acc, minlength=lib.K)[own].tolist()
    return acc


# ------------------------------------------------------------------------------------------------
# extraction: kmpgpu_load_frames (R1-R4, R6)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proto", ["udp", "tcp"])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, ROUND - 1, ROUND, ROUND + 1, GRID_ITEMS, GRID_ITEMS + 1, N_BIG])
def test_extraction_at_threshold_edges(gm, lib, proto, n):
    try:
        gm.set_patterns(lib.tags)
        kind = PM.make_sequence("mixed", n, lib.rule[proto][1], seed=n)
        acc = _check_extraction(gm, lib, proto, kind)
        assert len(acc) > n // 5
        if n > ROUND:
            assert len(acc) > GATHER_WAVES
    finally:
        reset(gm)


@pytest.mark.parametrize("proto", ["udp", "tcp"])
@pytest.mark.parametrize("shape", ["all_rejected", "last_only", "first_only", "empty_rounds", "all_empty"])
def test_extraction_sequence_shapes(gm, lib, proto, shape):
    """Shapes of the frame sequence at ten rounds of the totals kernel: carries through empty tiles and empty rounds, a single
    payload behind or before millions of rejected frames, 16-byte slots only."""
    try:
        gm.set_patterns(lib.tags)
        plen = lib.rule[proto][1]
        kind = PM.make_sequence(shape, N_BIG, plen, seed=11)
        acc = _check_extraction(gm, lib, proto, kind)
        if shape == "all_rejected":
            assert len(acc) == 0
            a2, off2, ln2 = gm.arena_download()
            assert len(off2) == len(ln2) == 0
            # a good batch right behind the empty one
            _check_extraction(gm, lib, proto, PM.make_sequence("mixed", 5000, plen, seed=12))
        elif shape in ("last_only", "first_only"):
            assert len(acc) == 1
        elif shape == "empty_rounds":
            ok = plen[kind] >= 0
            rounds = [bool(ok[r * ROUND:(r + 1) * ROUND].any()) for r in range(10)]
            assert rounds == [True, False, False, True, False, False, True, False, False, True]
        else:
            assert len(acc) > ROUND and int(plen[acc].max()) == 0
    finally:
        reset(gm)


def test_extraction_buffers_reused(gm, lib):
    """One context: a large batch, a small one, a large one in the two-step form.  The device buffers of the first are kept
    (kmpgpu_load_frames_finish); what the small batch leaves behind its end in them must not be counted or downloaded."""
    try:
        gm.set_patterns(lib.tags)
        plen = lib.rule["udp"][1]
        _check_extraction(gm, lib, "udp", PM.make_sequence("mixed", GRID_ITEMS + 1, plen, seed=21), packed_tags=False)
        _check_extraction(gm, lib, "udp", PM.make_sequence("mixed", TILE + 1, plen, seed=22))
        _check_extraction(gm, lib, "tcp", PM.make_sequence("empty_rounds", N_BIG, lib.rule["tcp"][1], seed=23), two_steps=True, packed_tags=False)
        _check_extraction(gm, lib, "udp", PM.make_sequence("mixed", 3, plen, seed=24))
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# past 4 GiB (R9)
# ------------------------------------------------------------------------------------------------
def _mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def test_arena_past_4_gib(gm, lib):
    """3.1 M payloads of 1 458 bytes: pkt_off crosses 2^32 (4.56 GB packed)."""
    poff, plen, payloads = lib.rule["udp"]
    big = np.flatnonzero(plen == 1458)
    assert len(big) >= 2
    n = 3_100_003
    rng = np.random.default_rng(31)
    kind = big[rng.integers(0, len(big), n)]
    rej = np.flatnonzero(plen < 0)
    kind[rng.integers(0, n, 1000)] = rej[0]                    # a few holes, so that payload number != frame number
    tag_ids = sorted(set(big.tolist()) | set(PM.own_tag_kinds(payloads)[:24]))
    try:
        gm.set_patterns([lib.tags[t] for t in tag_ids])
        n_pay = _load_frames(gm, lib.blob, lib.boff[kind], lib.cap[kind], "udp")
        acc, off, ln, src_off = PM.extraction_index(lib.boff, poff, plen, kind)
        slot = 1472
        end = int(off[-1]) + slot
        assert n_pay == len(acc) > 3_090_000 and end > (1 << 32) + (1 << 27)
        assert gm.arena_info() == (len(acc), 1458 * len(acc))
        a2, off2, ln2 = gm.arena_download()
        assert len(a2) == end + 64
        assert _first_diff(ln2, ln) is None and _first_diff(off2, off) is None
        k0 = int(np.searchsorted(off, 1 << 32))                # first payload at or behind 2^32
        assert off[k0 - 1] < (1 << 32) <= off[k0]
        ks = np.unique(np.concatenate([np.arange(0, 4096), np.arange(k0 - 2048, k0 + 2048), np.arange(len(acc) - 4096, len(acc)),
                                       rng.integers(0, len(acc), 4096)]))
        col = np.arange(slot, dtype=np.int64)
        got = a2[off[ks].astype(np.int64)[:, None] + col]
        want = lib.blob[np.minimum(src_off[ks][:, None] + col, len(lib.blob) - 1)]
        want[:, 1458:] = 0
        assert np.array_equal(got, want)
        del a2, got, want
        want_tags = np.bincount(acc, minlength=lib.K)[tag_ids]
        assert PM.tag_counts(payloads, acc, lib.K)[tag_ids].tolist() == want_tags.tolist()
        for kernel in (KERNEL_FUSED, KERNEL_PACKED, KERNEL_AUTO):
            assert _scan(gm, kernel).tolist() == want_tags.tolist(), kernel
        assert gm.effective_bytes() == 1458 * len(acc)
    finally:
        reset(gm)
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))      # gives the 4.6 GB back
    assert gm.arena_info() == (0, 0)


def test_source_past_4_gib(gm, lib):
    """A file buffer a little over 4 GiB with the library at its start, across the 2^32 boundary (one frame straddles it) and
    above it: file + frame_off[f] and src_off[k] as 64-bit values.  Skipped only where the host cannot hold the buffer."""
    if _mem_available() < (8 << 30):
        pytest.skip("MemAvailable is under 8 GiB")
    poff, plen, payloads = lib.rule["udp"]
    small = np.flatnonzero(plen <= 300)                        # rejected frames included
    j = int(max(k for k in small if plen[k] >= 100))           # this frame's copy straddles the boundary
    nb = len(lib.blob)
    base = np.array([0, (1 << 32) - int(lib.boff[j]) - 60, (1 << 32) + nb + 4096], dtype=np.uint64)
    assert base[1] + lib.boff[j] < (1 << 32) < base[1] + lib.boff[j] + lib.cap[j] and base[1] > nb
    buf = np.zeros((1 << 32) + 2 * nb + 8192, dtype=np.uint8)
    for b in base.tolist():
        buf[b:b + nb] = lib.blob
    n = 300_001
    rng = np.random.default_rng(32)
    kind = small[rng.integers(0, len(small), n)]
    copy = rng.integers(0, 3, n)
    kind[1000], copy[1000] = j, 1
    try:
        gm.set_patterns(lib.tags)
        n_pay = _load_frames(gm, buf, base[copy] + lib.boff[kind], lib.cap[kind], "udp")
        del buf
        acc, off, ln, arena = PM.extraction_arena(lib.blob, lib.boff, poff, plen, kind)
        assert n_pay == len(acc) > GATHER_WAVES and gm.arena_info() == (len(acc), int(ln.sum(dtype=np.uint64)))
        a2, off2, ln2 = gm.arena_download()
        assert _first_diff(ln2, ln) is None and _first_diff(off2, off) is None
        assert _first_diff(a2[:len(arena)], arena) is None
        want = PM.tag_counts(payloads, acc, lib.K)
        assert _scan(gm, KERNEL_FUSED).tolist() == want.tolist()
        assert gm.effective_bytes() == PM.effective_bytes(arena, off, ln)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# repack (R1-R4, R6, R8, R10)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [TILE + 1, ROUND + 1, 1_300_003])
def test_repack_at_scale(gm, oracle, n):
    """A caller's arena with shuffled slots, gaps and non-zero filler, uploaded (kmpgpu_load_arena) and borrowed
    (kmpgpu_attach_arena of torch tensors): repacked on the device, or scanned in place."""
    arena, off, ln = PM.shuffled_arena(n, seed=41)
    slot = PM.slot_bytes(ln)
    furthest = int(np.argmax(off + slot))
    if n > GRID_ITEMS:
        assert furthest >= SLOT_END_ITEMS                              # the furthest slot is found in a later round of kmp_slot_end_kernel
    new_off, packed = PM.gather_slots(arena, off, ln)
    pats = [b"ab", b"abcab", b"b", b"cabcabcabcab"]
    want, _ = oracle.count(arena, off, ln, pats, threads=8)
    assert oracle.count(packed, new_off, ln, pats, threads=8)[0].tolist() == want.tolist() and want[:3].min() > 0
    eff = PM.effective_bytes(arena, off, ln)
    assert eff < int(ln.sum(dtype=np.uint64))                          # NUL bytes are there
    d_arena = torch.from_numpy(arena).cuda(); d_off = torch.from_numpy(off.astype(np.int64)).cuda(); d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    try:
        for route in ("load", "attach"):
            for repack in (1, 0):
                gm.set_patterns(pats)
                gm.set_option(OPT_REPACK, repack)
                if route == "load":
                    gm.load_arena(arena, off, ln)
                else:
                    gm.attach_arena(d_arena, d_off, d_len)
                assert gm.arena_info() == (n, int(ln.sum(dtype=np.uint64)))
                for kernel in (KERNEL_AUTO, KERNEL_PACKED, KERNEL_FUSED, KERNEL_GENERAL):
                    assert _scan(gm, kernel).tolist() == want.tolist(), (route, repack, kernel)
                assert gm.effective_bytes() == eff
                a2, off2, ln2 = gm.arena_download()
                assert _first_diff(ln2, ln) is None
                if repack:
                    assert _first_diff(off2, new_off) is None
                    assert len(a2) == len(packed) + 64 and _first_diff(a2[:len(packed)], packed) is None and not a2[len(packed):].any()
                else:
                    assert _first_diff(off2, off) is None
                    assert len(a2) == len(arena) and _first_diff(a2, arena) is None                # untouched on the device
                    gm.set_option(OPT_KERNEL, KERNEL_AUTO); gm.set_option(OPT_FUSED, 2)
                    recs, found, counts = gm.scan_offsets(1024)                                    # packs on demand
                    assert found == int(want.sum()) and counts.tolist() == want.tolist() and len(recs) == 1024
                    for r in recs[::8]:
                        o = int(off[int(r["packet"])]) + int(r["offset"]); p = pats[int(r["pattern"])]
                        assert arena[o:o + len(p)].tobytes() == p and int(r["offset"]) + len(p) <= int(ln[int(r["packet"])])
                    # an all-nocase set on the arena in place: kmp_slot_end_kernel (borrowed route) and the fold
                    gm.set_patterns([b"AB", b"aBcAb", b"B", b"CABCABcabcab"], nocase=True)
                    if route == "load":
                        gm.load_arena(arena, off, ln)
                    else:
                        gm.attach_arena(d_arena, d_off, d_len)
                    for kernel in (KERNEL_AUTO, KERNEL_GENERAL):
                        assert _scan(gm, kernel).tolist() == want.tolist(), (route, "nocase", kernel)
                if route == "attach":
                    assert torch.equal(d_arena.cpu(), torch.from_numpy(arena)) and torch.equal(d_off.cpu(), torch.from_numpy(off.astype(np.int64)))
    finally:
        reset(gm)
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


# ------------------------------------------------------------------------------------------------
# slot padding (R5)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dirty_from", [0, PAD_ITEMS + 1])
def test_padding_at_scale(gm, oracle, dirty_from):
    """2.2 M payloads of 1..47 bytes whose slot padding continues the text (test_dirty_slot_padding's trap), in all slots or
    only in those behind the first grid-stride round of kmp_check_padding_kernel."""
    n = 2_200_000
    assert n > PAD_ITEMS + 100_000
    rng = np.random.default_rng(51)
    ln = rng.integers(1, 48, n).astype(np.uint32)
    slot = PM.slot_bytes(ln)
    off = PM.packed_offsets(ln)
    end = int(off[-1] + slot[-1])
    text = np.frombuffer((b"abc" * ((end + 64) // 3 + 1))[:end + 64], dtype=np.uint8)          # payload k = its slice of the period
    clean = PM.clean_padding(text, off, ln)
    clean[end:] = 0
    arena = text.copy()
    cut = int(off[dirty_from])
    arena[:cut] = clean[:cut]
    pats = [b"abc", b"abcabcabcabc", b"ab", b"c", b"cabca"]
    want, _ = oracle.count(arena, off, ln, pats, threads=8)
    assert oracle.count(clean, off, ln, pats, threads=8)[0].tolist() == want.tolist()
    overcount, _ = oracle.count(arena, off, slot.astype(np.uint32), pats, threads=8)
    assert overcount.sum() > want.sum()                                                       # the trap is armed
    try:
        gm.set_patterns(pats)
        gm.load_arena(arena, off, ln)                          # the context's own copy: padding cleared in place
        for kernel in (KERNEL_PACKED, KERNEL_FUSED, KERNEL_GENERAL):
            assert _scan(gm, kernel).tolist() == want.tolist(), ("owned", kernel)
        a2, off2, ln2 = gm.arena_download()
        assert _first_diff(off2, off) is None and _first_diff(ln2, ln) is None
        assert _first_diff(a2[:end], clean[:end]) is None      # every slot
        tail = int(off[n - 100_000])
        assert np.array_equal(a2[tail:end], clean[tail:end])   # ... the last 100 000 among them
        del a2
        d_arena = torch.from_numpy(arena).cuda(); d_off = torch.from_numpy(off.astype(np.int64)).cuda(); d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        gm.attach_arena(d_arena, d_off, d_len)                 # borrowed: left as it is
        for kernel in (KERNEL_PACKED, KERNEL_FUSED, KERNEL_GENERAL):
            assert _scan(gm, kernel).tolist() == want.tolist(), ("borrowed", kernel)
        assert np.array_equal(d_arena.cpu().numpy(), arena)
    finally:
        reset(gm)
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


# ------------------------------------------------------------------------------------------------
# kmpgpu_effective_bytes (R6)
# ------------------------------------------------------------------------------------------------
def test_effective_bytes_at_scale(gm):
    n = 100_003
    assert n > 3 * GATHER_WAVES
    rng = np.random.default_rng(61)
    ln = np.where(rng.random(n) < 0.5, rng.choice([0, 1, 15, 16, 17, 100, 1023, 1024, 1025, 1500, 4000, 5000], n), rng.integers(0, 5001, n)).astype(np.int64)
    off = PM.packed_offsets(ln).astype(np.int64)
    slot = PM.slot_bytes(ln).astype(np.int64)
    arena = rng.integers(1, 256, int(off[-1] + slot[-1]) + 64).astype(np.uint8)
    how = rng.integers(0, 5, n)                               # 0 none, 1 first byte, 2 last byte, 3 in the slot's last group, 4 anywhere (up to three)
    has = ln > 0
    arena[off[has & (how == 1)]] = 0
    arena[(off + ln - 1)[has & (how == 2)]] = 0
    g = has & (how == 3)
    lo = (ln - 1) // 16 * 16
    arena[(off + lo + rng.integers(0, 16, n) % (ln - lo).clip(1))[g]] = 0
    for _ in range(3):
        g = has & (how == 4) & (rng.random(n) < 0.7)
        arena[(off + rng.integers(0, 1 << 30, n) % ln.clip(1))[g]] = 0
    arena = PM.clean_padding(arena, off, ln)
    arena[int(off[-1] + slot[-1]):] = 0
    want = PM.effective_bytes(arena, off, ln)
    z = arena == 0
    brute = sum(int(np.argmax(z[o:o + l])) + 1 if z[o:o + l].any() else l for o, l in zip(off[:3000].tolist(), ln[:3000].tolist()))
    assert brute == PM.effective_bytes(arena, off[:3000], ln[:3000])
    assert want < int(ln.sum()) * 3 // 4
    gm.load_arena(arena, off.astype(np.uint64), ln.astype(np.uint32))
    try:
        assert gm.arena_info() == (n, int(ln.sum()))
        assert gm.effective_bytes() == want
    finally:
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


# ------------------------------------------------------------------------------------------------
# the device-side layout check (R7)
# ------------------------------------------------------------------------------------------------
N_IDX = 1_000_000


def _tiny_slots(seed=71):
    """1 M payloads of 1..16 bytes over {a, b} in 16-byte slots back to back."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(1, 17, N_IDX).astype(np.uint32)
    off = (np.arange(N_IDX, dtype=np.uint64) * np.uint64(16))
    arena = rng.integers(ord("a"), ord("b") + 1, 16 * N_IDX + 64).astype(np.uint8)
    arena = PM.clean_padding(arena, off, ln)
    arena[16 * N_IDX:] = 0
    return arena, off, ln


@pytest.mark.parametrize("where", [700_001, 0, N_IDX - 1])
def test_layout_check_on_the_device(gm, oracle, where):
    """One bad entry in an otherwise valid index of a borrowed arena, found by kmp_validate_index_kernel (the host never sees a
    device-resident index): refused with the matching message, nothing attached, and the context goes on with a good arena.
    The tensors are large enough for the bad entry too, and the told size covers no more than the tensor."""
    assert where in (0, N_IDX - 1) or where > VALIDATE_ITEMS + 75_000
    arena, off, ln = _tiny_slots()
    pats = [b"ab", b"bab"]
    want, _ = oracle.count(arena, off, ln, pats, threads=8)
    far = 16 * N_IDX                                             # behind every other slot
    d_big = torch.zeros(far + (1 << 30) + 64, dtype=torch.uint8, device="cuda")
    d_big[:len(arena)] = torch.from_numpy(arena).cuda()
    d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    cases = []
    o = off.copy(); o[where] += np.uint64(8)
    cases.append(("not 16-byte aligned", o, ln, far + 64))
    o = off.copy(); o[where] = far                               # its slot [far, far + 16) ends one byte behind the arena
    cases.append(("exceeds the arena", o, ln, far + 15))
    o = off.copy(); o[where] = far
    l = ln.copy(); l[where] = (1 << 30) + 1                       # 2^30 itself is the longest payload (a stream cut at KMPGPU_STREAM_DEPTH_MAX)
    cases.append(("above 2^30", o, l, far + (1 << 30) + 64))
    try:
        gm.set_patterns(pats)
        for msg, o, l, told in cases:
            assert told <= d_big.numel()
            d_o = torch.from_numpy(o.astype(np.int64)).cuda(); d_l = torch.from_numpy(l.astype(np.int32)).cuda()
            torch.cuda.synchronize()
            with pytest.raises(KmpGpuError) as e:
                gm.attach_arena(d_big, d_o, d_l, arena_bytes=told)
            assert msg in str(e.value) and "(-2)" in str(e.value), str(e.value)               # KMPGPU_EINVAL
            assert gm.arena_info() == (0, 0)                     # nothing attached: a scan has no index to touch
            assert gm.scan()[0].tolist() == [0, 0]
            gm.attach_arena(d_big, d_off, d_len, arena_bytes=far + 64)
            assert gm.arena_info() == (N_IDX, int(ln.sum(dtype=np.uint64)))
            assert _scan(gm, KERNEL_AUTO).tolist() == want.tolist()
        # the entry moved to the far end with its length kept is legal (a gap where it was): attached, repacked, counted
        o = off.copy(); o[where] = far
        d_o = torch.from_numpy(o.astype(np.int64)).cuda()
        d_big[far:far + 16] = d_big[16 * where:16 * where + 16]
        torch.cuda.synchronize()
        gm.attach_arena(d_big, d_o, d_len, arena_bytes=far + 16)
        assert _scan(gm, KERNEL_AUTO).tolist() == want.tolist()
    finally:
        reset(gm)
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


@pytest.mark.parametrize("route", ["attach", "load"])
def test_uniform_index_with_one_odd_length(gm, oracle, route):
    """All payloads 12 bytes in 16-byte slots but one of 5 bytes at entry 700 001 whose slot still holds the text: the index
    is not uniform, so the flat kernel's arithmetic (offset = k * stride, one length for all) must not be taken."""
    n, odd = N_IDX, 700_001
    assert odd > VALIDATE_ITEMS
    ln = np.full(n, 12, dtype=np.uint32)
    ln[odd] = 5
    off = np.arange(n, dtype=np.uint64) * np.uint64(16)
    arena = np.frombuffer(b"xxxxxxabxxxx\0\0\0\0" * n + b"\0" * 64, dtype=np.uint8).copy()
    pats = [b"ab", b"xab"]
    want, _ = oracle.count(arena, off, ln, pats, threads=8)
    assert want.tolist() == [n - 1, n - 1]
    d = (torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    try:
        gm.set_patterns(pats)
        if route == "attach":
            gm.attach_arena(*d)
        else:
            gm.load_arena(arena, off, ln)
        assert gm.arena_info() == (n, 12 * n - 7)
        for kernel in (KERNEL_AUTO, KERNEL_PACKED, KERNEL_FUSED, KERNEL_GENERAL):
            assert _scan(gm, kernel).tolist() == want.tolist(), kernel
    finally:
        reset(gm)
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


# ------------------------------------------------------------------------------------------------
# one context through every loader: the kept buffers grow, are reused, and carry no arena over
# ------------------------------------------------------------------------------------------------
def _mixed_arena(n, seed):
    """n payloads of 0..200 bytes over the letters of the two patterns below, packed, padding 0x00."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, 201, n).astype(np.uint32)
    off = PM.packed_offsets(ln)
    end = int(off[-1] + PM.slot_bytes(ln)[-1]) if n else 0
    arena = np.frombuffer(b"idhtp", dtype=np.uint8)[rng.integers(0, 5, end + 64)]
    arena = PM.clean_padding(arena, off, ln)
    arena[end:] = 0
    return arena, off.astype(np.uint64), ln


def test_one_context_through_every_loader(oracle):
    """kmpgpu_load_arena, kmpgpu_attach_arena, kmpgpu_load_frames and kmpgpu_load_selected share the context's arena buffers and
    one way of installing an arena: sizes that grow and shrink in a fixed order, and after every step the arena's size and the
    counts of two patterns against the oracle.  Then the uploads again on a context whose buffers kmpgpu_reserve took first."""
    import os

    from conftest import DATA
    from multithreading_string_matching_amd.host import HostArena

    pats = [b"id", b"http"]
    pcap = os.path.join(DATA, "udp.pcap")
    cap = HostArena.from_pcap(pcap, "udp")
    arenas = {n: _mixed_arena(n, seed=80 + k) for k, n in enumerate((300, 3000, 100))}
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    want = {n: oracle.count(a, off, ln, pats)[0].tolist() for n, (a, off, ln) in arenas.items()}
    want_cap = oracle.count(cap.bytes, cap.off, cap.len, pats)[0].tolist()
    assert min(want[300]) > 0 and min(want_cap) > 0
    sel = np.arange(300) % 3 == 1                                       # every third payload of the 300
    a, off, ln = arenas[300]
    s_off, s_arena = PM.gather_slots(a, off[sel], ln[sel])
    want_sel = oracle.count(s_arena, s_off, ln[sel], pats)[0].tolist()
    d300 = (torch.from_numpy(a).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()

    def check(m, n_pkts, payload_bytes, counts, step):
        assert m.arena_info() == (n_pkts, payload_bytes), step
        for kernel in (KERNEL_AUTO, KERNEL_PACKED):
            assert _scan(m, kernel).tolist() == counts, (step, kernel)

    def upload(m, n, step):
        m.load_arena(*arenas[n])
        check(m, n, int(arenas[n][2].sum()), want[n], step)

    def frames(m, step):
        assert m.load_pcap_frames(pcap, "udp")[0] == int(cap.len.shape[0])
        check(m, int(cap.len.shape[0]), int(cap.len.sum()), want_cap, step)

    with GpuMatcher(0) as m, GpuMatcher(0) as src, GpuMatcher(0) as r:
        for x in (m, src, r):
            x.set_patterns(pats)
        src.load_arena(*arenas[300])
        upload(m, 300, "load 300")
        m.attach_arena(*d300)                                           # borrowed: the context's own buffers are given back
        check(m, 300, int(ln.sum()), want[300], "attach 300")
        upload(m, 3000, "load 3000 (the buffers grow)")
        upload(m, 100, "load 100 (the buffers are reused)")
        frames(m, "frames")
        assert m.load_selected(src, sel).tolist() == np.flatnonzero(sel).tolist()
        check(m, int(sel.sum()), int(ln[sel].sum()), want_sel, "selected")
        m.load_arena(*empty)
        check(m, 0, 0, [0, 0], "empty")
        upload(m, 300, "load 300 again")

        big = arenas[3000]
        _lib.gpu_check(_lib.gpu_lib().kmpgpu_reserve(r._ctx, big[0].size, 3000, os.path.getsize(pcap), 4096), "kmpgpu_reserve")
        assert r.arena_info() == (0, 0)
        for n in (300, 3000, 100):
            upload(r, n, f"reserved, load {n}")
        frames(r, "reserved, frames")
        r.load_arena(*empty)
        check(r, 0, 0, [0, 0], "reserved, empty")
        upload(r, 300, "reserved, load 300 again")
