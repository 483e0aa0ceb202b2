"""Case-insensitive patterns (KMPGPU_PAT_NOCASE, kmpgpu_set_patterns_flags) on a real MI355X.

The checker is the CPU oracle, unchanged, applied to host-folded inputs (oracle_counts_arena of tests/match_model.py): for a
nocase pattern p, count(payloads, p) == oracle.count(fold(payloads), fold(p)).  Offset records come from the host model there.

Run on a real MI355X:  python -m pytest tests/test_gpu_nocase.py -m gpu
"""
import os
import random

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import VARIANTS, gm, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_FLAT, KERNEL_GENERAL, KERNEL_PACKED, OPT_ACCUMULATE, OPT_FUSED, OPT_KERNEL, OPT_MODE, OPT_REPACK, PAT_NOCASE)

# letters of both cases, the bytes next to 'A'..'Z' / 'a'..'z', and their bit-7 twins (0xC1 / 0xE1 are 'A' / 'a' + 0x80)
ALPHABET = b"aAbBcCzZ@[`{" + bytes([0xC1, 0xE1, 0xDA, 0xFA])
FIXTURE_KEYS = ["udp.pcap:udp", "udp_1000.pcap:udp", "big_udp.pcap:udp", "very_big_udp.pcap:udp",
                "tcp.pcap:tcp", "tcp.pcap:udp", "udp.pcap:tcp", "udp_1000.pcap:tcp"]


def random_case(rng, p):
    return bytes(c ^ 0x20 if (0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A) and rng.random() < 0.5 else c for c in p)


def random_payloads(rng, n, length=None, nul=0.2):
    out = []
    for _ in range(n):
        L = length if length is not None else rng.randrange(0, 2200)
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        if L and rng.random() < nul:
            b[rng.randrange(L)] = 0
        out.append(bytes(b))
    return out


def patterns_from(rng, payloads, lengths):
    """Substrings of the payloads (so that they match), in random case, plus a few random ones."""
    pats = []
    for m in lengths:
        for _ in range(2):
            for _ in range(100):
                t = payloads[rng.randrange(len(payloads))]
                if len(t) >= m:
                    s = rng.randrange(len(t) - m + 1)
                    p = t[s:s + m]
                    if 0 not in p:
                        pats.append(random_case(rng, p))
                        break
            else:
                pats.append(bytes(rng.choice(ALPHABET) for _ in range(m)))
    return pats


LENGTHS = [1, 2, 3, 4, 8, 9, 16, 17, 40, 99]


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_kernel_family(gm, oracle, uniform, variant):
    name, mode, kernel, fused = variant
    rng = random.Random(101 + 7 * uniform + len(name))
    payloads = random_payloads(rng, 600, length=1500 if uniform else None)
    pats = patterns_from(rng, payloads, LENGTHS) + [b"A", b"@", b"\xc1", b"Z"]     # 1-byte patterns ride along with the fused pass
    arena = K.HostArena.from_payloads(payloads)
    want = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, True)
    want_cs = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, False)
    assert want != want_cs                           # the input tells the two apart
    reset(gm)
    gm.set_option(OPT_MODE, mode); gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
    gm.set_patterns(pats, nocase=True)
    gm.load_arena(arena)
    assert gm.scan()[0].tolist() == want, name
    assert gm.scan()[0].tolist() == want, name      # a repeat scan (the fold is not redone)
    gm.set_patterns(pats)                            # the same context, case-sensitive again
    assert gm.scan()[0].tolist() == want_cs, name
    reset(gm)


@pytest.mark.parametrize("n_pats", [300, 1100])
def test_classed_groups(gm, oracle, n_pats):
    """More than 256 distinct nocase patterns: the fused pass's classed groups, built on folded keys."""
    rng = random.Random(n_pats)
    payloads = random_payloads(rng, 800)
    pats = patterns_from(rng, payloads, [rng.randrange(3, 12) for _ in range(n_pats // 2)])[:n_pats]
    arena = K.HostArena.from_payloads(payloads)
    want = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, True)
    reset(gm)
    gm.set_patterns(pats, nocase=True)
    gm.load_arena(arena)
    for fused in (1, 0):
        gm.set_option(OPT_FUSED, fused)
        assert gm.scan()[0].tolist() == want, fused
    reset(gm)


def test_mixed_flags_in_one_set(gm, oracle):
    rng = random.Random(5)
    words = [b"Host", b"host", b"HOST", b"hOsT", b"GET", b"get", b"User-Agent", b"@[`{", b"12", b"\xc1\xda"]
    payloads = []
    for _ in range(500):
        parts = [random_case(rng, rng.choice(words)) if rng.random() < 0.5 else bytes(rng.choice(ALPHABET) for _ in range(rng.randrange(0, 30)))
                 for _ in range(rng.randrange(0, 40))]
        payloads.append(b" ".join(parts))
    pats = [b"Host", b"host", b"HOST", b"hOsT", b"Host", b"host", b"GET", b"get", b"user-agent", b"@[`{", b"12", b"\xc1\xda", b"H", b"t"]
    flags = [False, True, True, True, True, False, False, True, True, True, True, True, True, False]
    arena = K.HostArena.from_payloads(payloads)
    want = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, flags)
    assert want[0] != want[1] and want[1] == want[2] == want[3] == want[4]
    reset(gm)
    gm.load_arena(arena)
    for fused in (2, 0):
        gm.set_option(OPT_FUSED, fused)
        gm.set_patterns(pats, nocase=flags)
        assert gm.scan()[0].tolist() == want, fused
    reset(gm)

    # nocase patterns without a letter are their case-sensitive selves: no fold, no second read
    plain = [b"@[`{", b"12", b"\xc1\xda", b"{", b"``@"]
    gm.set_patterns(plain)
    got_cs, t_cs = gm.scan()
    gm.set_patterns(plain, nocase=True)
    got_nc, t_nc = gm.scan()
    assert got_nc.tolist() == got_cs.tolist() == MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, plain, False)
    assert t_nc.launches == t_cs.launches


@pytest.mark.parametrize("key", FIXTURE_KEYS)
def test_strings_txt_nocase_still_fuses(gm, oracle, tokens, key):
    pcap, mode = key.split(":")
    arena = K.HostArena.from_pcap(os.path.join(DATA, pcap), mode)
    want = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, tokens, True)
    reset(gm)
    gm.load_arena(MM.fold(arena.bytes), arena.off, arena.len)      # the host-folded formulation: folded arena, folded tokens, case-sensitive
    gm.set_patterns([MM.fold(t) for t in tokens])
    got_f, t_f = gm.scan()
    gm.load_arena(arena)
    gm.set_patterns(tokens, nocase=True)
    got, t = gm.scan()
    assert got.tolist() == want == got_f.tolist()
    assert t.launches == t_f.launches and t.grid_blocks == t_f.grid_blocks


@pytest.mark.parametrize("uniform", [False, True])
def test_offsets_mixed_set(gm, oracle, uniform):
    rng = random.Random(41 + uniform)
    payloads = random_payloads(rng, 400, length=1500 if uniform else None)
    pats = [b"aB", b"ab", b"AbC", b"@[", b"\xc1a", b"zZzZ", b"b", b"A", b"Ab"] + patterns_from(rng, payloads, [5, 17])
    flags = [True, False, True, True, True, True, False, True, True] + [i % 2 == 0 for i in range(4)]
    want = sorted(MM.records(MM.starts(payloads, pats, nocase=flags)))
    arena = K.HostArena.from_payloads(payloads)
    counts_want = MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, flags)
    assert len(want) == sum(counts_want)
    reset(gm)
    gm.set_patterns(pats, nocase=flags)
    gm.load_arena(arena)
    for kernel, fused in ((KERNEL_AUTO, 0), (KERNEL_PACKED, 0), (KERNEL_FLAT, 0), (KERNEL_AUTO, 1)):
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        got, found, counts = gm.scan_offsets(len(want) + 10)
        assert found == len(want) and counts.tolist() == counts_want, (kernel, fused)
        assert MM.triples(got) == want, (kernel, fused)
    reset(gm)


def test_arena_untouched_and_no_stale_fold(gm, oracle):
    rng = random.Random(77)
    pats = [b"Ab", b"aBc@", b"zz", b"CaB" * 5]
    a = K.HostArena.from_payloads(random_payloads(rng, 500, length=900))
    b = K.HostArena.from_payloads(random_payloads(rng, 500, length=900))
    assert a.nbytes == b.nbytes
    reset(gm)
    gm.set_patterns(pats, nocase=True)
    gm.load_arena(a)
    assert gm.scan()[0].tolist() == MM.oracle_counts_arena(oracle, a.bytes, a.off, a.len, pats, True)
    got, off, ln = gm.arena_download()                 # the original bytes, not the folded copy
    end = int(off[-1]) + max(16, (int(ln[-1]) + 15) // 16 * 16)
    assert np.array_equal(got[:end], np.asarray(a.bytes)[:end])
    gm.set_patterns(pats)
    assert gm.scan()[0].tolist() == MM.oracle_counts_arena(oracle, a.bytes, a.off, a.len, pats, False)
    gm.set_patterns(pats, nocase=True)
    gm.load_arena(b)                                   # same size: into the same device buffers
    assert gm.scan()[0].tolist() == MM.oracle_counts_arena(oracle, b.bytes, b.off, b.len, pats, True)


def test_borrowed_arena_rewritten_and_reattached(gm, oracle):
    import torch
    rng = random.Random(9)
    pats = [b"aB", b"ABCA", b"abcABCabcABCab", b"\xe1"]
    first = K.HostArena.from_payloads(random_payloads(rng, 400))
    second = K.HostArena.from_payloads(random_payloads(rng, 900, nul=0.0))
    cap = max(first.nbytes, second.nbytes)
    d_arena = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(max(first.n_pkts, second.n_pkts), dtype=torch.int64, device="cuda")
    d_len = torch.zeros(max(first.n_pkts, second.n_pkts), dtype=torch.int32, device="cuda")
    gm.set_stream(None)
    reset(gm)
    gm.set_patterns(pats, nocase=True)
    for a in (first, second, first):
        d_arena.zero_()
        d_arena[: a.nbytes] = torch.from_numpy(np.array(a.bytes))
        d_off[: a.n_pkts] = torch.from_numpy(a.off.astype(np.int64))
        d_len[: a.n_pkts] = torch.from_numpy(a.len.astype(np.int32))
        torch.cuda.synchronize()
        gm.attach_arena(d_arena, d_off[: a.n_pkts], d_len[: a.n_pkts])
        want = MM.oracle_counts_arena(oracle, a.bytes, a.off, a.len, pats, True)
        for fused in (0, 1):
            gm.set_option(OPT_FUSED, fused)
            assert gm.scan()[0].tolist() == want
    reset(gm)
    host = d_arena.cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(host[: first.nbytes], np.asarray(first.bytes))     # the borrowed arena was never written


def test_non_packed_arena_in_place(gm, oracle):
    """A shuffled index with gaps, scanned in place (KMPGPU_OPT_REPACK = 0): the fold covers up to the furthest slot, which
    is not the last entry's."""
    rng = random.Random(17)
    payloads = random_payloads(rng, 500, nul=0.1)
    payloads = [p[: rng.randrange(0, 700)] for p in payloads]
    order = list(range(len(payloads)))
    rng.shuffle(order)
    off = np.zeros(len(payloads), dtype=np.uint64)
    pos = 0
    for k in order:
        pos += 16 * rng.randrange(0, 4)
        off[k] = pos
        pos += max(16, (len(payloads[k]) + 15) // 16 * 16)
    assert int(off[-1]) + 16 < pos                    # the last entry is not the furthest slot
    arena = np.full(pos + 64, ord("B"), dtype=np.uint8)
    for k, p in enumerate(payloads):
        arena[int(off[k]):int(off[k]) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    ln = np.array([len(p) for p in payloads], dtype=np.uint32)
    pats = [b"aB", b"abCab", b"b", b"CABcabCABcab", b"@a"]
    want = MM.oracle_counts_arena(oracle, arena, off, ln, pats, True)
    reset(gm)
    gm.set_patterns(pats, nocase=True)
    for repack in (1, 0):
        gm.set_option(OPT_REPACK, repack)
        gm.load_arena(arena, off, ln)
        for kernel in (KERNEL_AUTO, KERNEL_PACKED, KERNEL_GENERAL):
            gm.set_option(OPT_KERNEL, kernel)
            assert gm.scan()[0].tolist() == want, (repack, kernel)
        if not repack:
            gm.set_option(OPT_KERNEL, KERNEL_AUTO)
            recs, found, counts = gm.scan_offsets(sum(want) + 4)         # packs the arena on demand: folded again
            assert found == sum(want) and counts.tolist() == want
            assert MM.triples(recs) == \
                sorted(MM.records(MM.starts(payloads, pats, nocase=[True] * len(pats))))
            assert gm.scan()[0].tolist() == want
    reset(gm)


def test_accumulate_over_batches(gm, oracle):
    rng = random.Random(3)
    pats = [b"aB", b"AbCaB", b"c", b"\xc1", b"Host"]
    batches = [random_payloads(rng, 300) for _ in range(3)]
    want = [0] * len(pats)
    for bt in batches:
        a = K.HostArena.from_payloads(bt)
        want = [x + y for x, y in zip(want, MM.oracle_counts_arena(oracle, a.bytes, a.off, a.len, pats, True))]
    reset(gm)
    gm.set_patterns(pats, nocase=True)
    gm.set_option(OPT_ACCUMULATE, 1)
    gm.counts_reset()
    for bt in batches:
        gm.load_arena(K.HostArena.from_payloads(bt))
        got = gm.scan()[0]
    reset(gm)
    assert got.tolist() == want


@pytest.mark.parametrize("key", ["udp_1000.pcap:udp", "tcp.pcap:tcp", "big_udp.pcap:udp", "udp.pcap:tcp"])
def test_device_extraction(gm, oracle, tokens, key):
    pcap, mode = key.split(":")
    path = os.path.join(DATA, pcap)
    host = K.HostArena.from_pcap(path, mode)
    reset(gm)
    gm.set_patterns(tokens, nocase=True)
    gm.load_pcap_frames(path, mode)
    assert gm.scan()[0].tolist() == MM.oracle_counts_arena(oracle, host.bytes, host.off, host.len, tokens, True)


def test_api_flags(gm, oracle, tokens):
    import ctypes as C
    u8p = C.POINTER(C.c_uint8)
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    reset(gm)
    gm.load_arena(arena)
    gm.set_patterns(tokens)
    want, t_want = gm.scan()
    n = len(tokens)
    bufs = [np.frombuffer(p + b"\0", dtype=np.uint8) for p in tokens]
    ptrs = (u8p * n)(*[b.ctypes.data_as(u8p) for b in bufs])
    lens = (C.c_uint32 * n)(*[len(p) for p in tokens])
    g = _lib.gpu_lib()
    assert g.kmpgpu_set_patterns_flags(gm._ctx, ptrs, lens, None, n) == 0          # flags = NULL
    got, t = gm.scan()
    assert got.tolist() == want.tolist() and t.launches == t_want.launches
    for bad in (2, 0x80000000, PAT_NOCASE | 4):
        flags = (C.c_uint32 * n)(*([0] * (n - 1) + [bad]))
        assert g.kmpgpu_set_patterns_flags(gm._ctx, ptrs, lens, flags, n) == -2        # KMPGPU_EINVAL
        assert b"flag" in g.kmpgpu_last_error()
    gm.set_patterns(tokens, nocase=True)                                                # the context is still usable
    assert gm.scan()[0].tolist() == MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, tokens, True)
    with pytest.raises(ValueError):
        gm.set_patterns(tokens, nocase=[True])


# ------------------------------------------------------------------------------------------------
# the drop-in command lines: KMPGPU_NOCASE=1
# ------------------------------------------------------------------------------------------------
CLI_RUNS = [("serial", [], {}), ("openmp_data", ["2"], {}), ("openmp_task", ["2"], {"KMPGPU_DEVICE_EXTRACT": "0", "KMPGPU_BATCH_BYTES": "65536"}),
            ("openmp_task", ["1"], {"KMPGPU_DEVICE_EXTRACT": "1", "KMPGPU_BATCH_BYTES": "65536"}), ("serial", [], {"KMPGPU_DEVICE_EXTRACT": "1"})]


@pytest.mark.parametrize("key", ["udp_1000.pcap:udp", "tcp.pcap:tcp"])
@pytest.mark.parametrize("run", CLI_RUNS, ids=[f"{r[0]}-{i}" for i, r in enumerate(CLI_RUNS)])
def test_cli_nocase(oracle, tokens, key, run):
    prog, extra, env_extra = run
    pcap, mode = key.split(":")
    host = K.HostArena.from_pcap(os.path.join(DATA, pcap), mode)
    want = MM.oracle_counts_arena(oracle, host.bytes, host.off, host.len, tokens, True)
    assert want != MM.oracle_counts_arena(oracle, host.bytes, host.off, host.len, tokens, False)
    r = run_cli(prog, pcap, extra=extra, env_extra=dict(env_extra, KMPGPU_NOCASE="1"), mode=mode, scrub=None)
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == K.format_report(tokens, want)


def test_cli_offsets_file_nocase(oracle, tokens, tmp_path):
    host = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [host.payload(k) for k in range(host.n_pkts)]
    want = sorted(MM.records(MM.starts(payloads, tokens, nocase=[True] * len(tokens))))
    out = tmp_path / "offsets.csv"
    r = run_cli("serial", env_extra={"KMPGPU_NOCASE": "1", "KMPGPU_OFFSETS_FILE": str(out)}, scrub=None)
    assert r.returncode == 0, r.stderr
    got = sorted(tuple(int(x) for x in line.split(",")) for line in out.read_text().splitlines() if line and line[0].isdigit())
    assert got == want


# ------------------------------------------------------------------------------------------------
# full size: 8 M x 1500 B (12 GB, a fold past 4 GiB), closed form
# ------------------------------------------------------------------------------------------------
def test_full_size_8m_shard(gm):
    import torch
    needle = b"NEEDLE_16B_PATRN"
    sp = K.SynthParams.make(seed=1234, needle=needle, plant_permille=100)        # lowercase text, the needle as written
    n, first, stride = 8_000_000, 5 * 8_000_000, 1504
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gm.set_stream(None)
    gm.fixed_index(d_off, d_len, 1500, 16)
    gm.synth_fill(d_arena, d_off, d_len, sp, first_pkt_id=first)
    gm.sync()
    planted = K.synth_count_planted(sp, n, 1500, first_pkt_id=first)
    assert planted > 0
    reset(gm)
    pats = [b"needle_16b_PATRN", b"needle_16b_patrn", b"ABCD", b"abcd"]
    gm.set_patterns(pats, nocase=[True, False, True, False])
    gm.attach_arena(d_arena, d_off, d_len)
    got, t = gm.scan()
    # '_', '1' and '6' occur only in the needle: the nocase needle matches exactly the planted ones
    assert int(got[0]) == planted and int(got[1]) == 0 and int(got[2]) == int(got[3]) > 0
    gm.set_patterns(pats[:1], nocase=True)
    assert int(gm.scan()[0][0]) == planted
    del d_arena, d_off, d_len
    torch.cuda.empty_cache()
