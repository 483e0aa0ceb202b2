"""Which payloads hold which patterns (kmpgpu_scan_packets, GpuMatcher.scan_packets) on a real MI355X.

The expectation is the hit matrix of the host model (tests/match_model.py); the totals come from the CPU oracle.  Every output of
the call is compared exactly: pkt_counts, any, the hit matrix and counts.

Run on a real MI355X:  python -m pytest tests/test_gpu_packets.py -m gpu
"""
import os
import random

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import KERNELS, gm, load, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import torch  # noqa: E402

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_GENERAL, MODE_AUTOMATON, OPT_ACCUMULATE, OPT_FUSED, OPT_KERNEL, OPT_MODE, OPT_REPACK, GpuMatcher)

ALPHABET = b"abcdAB"


def check(res, hits, counts):
    n_pat, n_pkts = hits.shape
    assert res["hits"].shape == (n_pat, n_pkts)
    bad = np.argwhere(res["hits"] != hits)
    assert bad.size == 0, [(int(i), int(k), bool(hits[i, k])) for i, k in bad[:8]]
    assert res["pkt_counts"].tolist() == hits.sum(axis=1).tolist()
    assert res["any"].tolist() == hits.any(axis=0).tolist()
    assert res["counts"].tolist() == list(counts)
    pc, c = res["pkt_counts"], res["counts"]
    assert (pc <= c).all() and ((pc == 0) == (c == 0)).all()


# ------------------------------------------------------------------------------------------------
# 1 + 2. random arenas x pattern sets x kernels
# ------------------------------------------------------------------------------------------------
def _arena(rng, kind, plant):
    """(payloads, slot bytes or None): the slot bytes hold the payloads AND what lies in their padding (kind "dirty")."""
    n = 300
    if kind == "uniform":
        lens = [1500] * n
    elif kind == "empty":
        lens = [0 if rng.random() < 0.5 else rng.randrange(0, 700) for _ in range(n)]
    else:
        lens = [rng.randrange(0, 2200) for _ in range(n)]
    payloads = []
    for L in lens:
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        for _ in range(L // 150):                    # plant patterns so that most of them hit somewhere
            p = rng.choice(plant)
            if len(p) <= L:
                s = rng.randrange(L - len(p) + 1)
                b[s:s + len(p)] = p
        if kind == "nul" and L and rng.random() < 0.5:
            b[rng.randrange(L)] = 0
        payloads.append(bytes(b))
    if kind != "dirty":
        return payloads, None
    # the padding continues with text that would complete a match: a kernel that read past a payload's end would overcount
    slots = []
    for t in payloads:
        pad = (-len(t)) % 16 or (16 if not t else 0)
        p = rng.choice(plant)
        slots.append(t + (p * (pad // max(len(p), 1) + 1))[:pad])
    return payloads, slots


def _sub(rng, payloads, m):
    """a piece of some payload's text (so that it matches), or random bytes"""
    for _ in range(200):
        t = rng.choice(payloads)
        t = t[:MM.text_end(t)]
        if len(t) >= m:
            s = rng.randrange(len(t) - m + 1)
            return t[s:s + m]
    return bytes(rng.choice(ALPHABET) for _ in range(m))


def _pattern_set(rng, name, payloads, tokens):
    """(patterns, nocase flags)"""
    def sub(m):
        return _sub(rng, payloads, m)
    if name == "riders":
        pats = [b"a", b"B", b"c", b"d", b"A", sub(5), sub(9), sub(3), sub(2)]      # four 1-byte riders, a fifth keeps a pass of its own
    elif name == "tokens":
        pats = list(tokens)
    elif name == "classed":
        seen, pats = set(), []
        while len(pats) < 300:
            p = sub(rng.choice([4, 5, 6, 8]))
            if p not in seen and b"\0" not in p:
                seen.add(p); pats.append(p)
    elif name == "dups":
        base = [sub(3), sub(7), sub(17), b"ab", b"b"]
        pats = base + [base[1], base[3], base[4], base[1]]
    elif name == "nocase":
        pats = [sub(m) for m in (1, 2, 4, 6, 16, 17)] + [b"ABab", b"aBc", b"b"]
        return pats, [rng.random() < 0.5 for _ in pats]
    else:
        raise AssertionError(name)
    return [p.replace(b"\0", b"a") for p in pats], None


SINGLE_LENGTHS = [1, 2, 3, 4, 16, 17, 99]
ARENAS = ["uniform", "mixed", "dirty", "nul", "empty"]
SETS = ["singles", "riders", "tokens", "classed", "dups", "nocase"]


@pytest.mark.parametrize("pset", SETS)
@pytest.mark.parametrize("kind", ARENAS)
def test_random_arenas(gm, oracle, tokens, kind, pset):
    rng = random.Random(f"{kind}-{pset}")
    plant = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (2, 4, 16, 17, 40)] + list(tokens[:20])
    if pset == "singles":
        payloads, slots = _arena(rng, kind, plant + [b"ab" * 50])
        sets = [([(b"ab" * 50)[:m] if m == 99 else _sub(rng, payloads, m).replace(b"\0", b"a")], None) for m in SINGLE_LENGTHS]
    else:
        payloads, slots = _arena(rng, kind, plant)
        sets = [_pattern_set(rng, pset, payloads, tokens)]
    keep = load(gm, payloads, slots)
    try:
        for pats, nocase in sets:
            hits = MM.hits(MM.starts(payloads, pats, nocase=nocase))
            counts = MM.oracle_counts(oracle, payloads, pats, nocase)
            gm.set_patterns(pats, nocase=nocase if nocase else False)
            for name, kernel, fused in KERNELS:
                reset(gm)
                gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
                res = gm.scan_packets(hits=True)
                check(res, hits, counts)
                assert gm.scan()[0].tolist() == counts, name
            # 2. the hit matrix = the distinct (packet, pattern) pairs of the offset records
            reset(gm)
            total = sum(counts)
            recs, found, _ = gm.scan_offsets(total)
            assert found == total
            pairs = {(int(r["pattern"]), int(r["packet"])) for r in recs}
            assert pairs == {(int(i), int(k)) for i, k in np.argwhere(hits)}
    finally:
        reset(gm)
        del keep


# ------------------------------------------------------------------------------------------------
# 3. the capture fixtures x strings.txt
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["udp", "tcp"])
@pytest.mark.parametrize("pcap", ["udp.pcap", "udp_1000.pcap", "big_udp.pcap", "very_big_udp.pcap", "tcp.pcap"])
def test_pcap_fixtures(gm, oracle, tokens, pcap, mode):
    arena = K.HostArena.from_pcap(os.path.join(DATA, pcap), mode)
    payloads = [arena.payload(k) for k in range(arena.n_pkts)]
    hits = MM.hits(MM.starts(payloads, tokens), len(tokens))
    counts = MM.oracle_counts(oracle, payloads, tokens)
    reset(gm)
    gm.set_patterns(tokens)
    gm.load_arena(arena)
    res = gm.scan_packets(hits=True)
    check(res, hits, counts)
    assert res["timing"].launches >= 1 if arena.n_pkts else res["timing"].launches == 0
    # the outputs the caller leaves out: NULL pointers through the C-ABI
    g = _lib.gpu_lib()
    pc = np.zeros(len(tokens), dtype=np.uint64)
    assert g.kmpgpu_scan_packets(gm._ctx, pc.ctypes.data, None, None, None, None) == 0
    assert pc.tolist() == hits.sum(axis=1).tolist()


# ------------------------------------------------------------------------------------------------
# 4. context state
# ------------------------------------------------------------------------------------------------
def test_context_state(gm, oracle):
    rng = random.Random(4)
    pats = [b"ab", b"abcab", b"b", b"aBcd", b"ab"]
    big = [bytes(rng.choice(b"abcd") for _ in range(rng.randrange(0, 900))) for _ in range(2000)]
    small = [bytes(rng.choice(b"abcd") for _ in range(rng.randrange(0, 300))) for _ in range(70)]
    g = _lib.gpu_lib()
    try:
        reset(gm)
        gm.set_patterns(pats)
        # running totals under OPT_ACCUMULATE are left alone
        gm.load_arena(K.HostArena.from_payloads(big))
        want_big = MM.oracle_counts(oracle, big, pats)
        hits_small, want_small = MM.hits(MM.starts(small, pats)), MM.oracle_counts(oracle, small, pats)
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        gm.scan_enqueue(); gm.scan_enqueue()
        assert gm.counts_read().tolist() == [2 * c for c in want_big]
        check(gm.scan_packets(hits=True), MM.hits(MM.starts(big, pats)), want_big)
        assert gm.counts_read().tolist() == [2 * c for c in want_big]
        gm.set_option(OPT_ACCUMULATE, 0)
        assert gm.scan()[0].tolist() == want_big                      # a later scan() still matches
        # a smaller arena after a larger one: no stale bits, no stale totals
        gm.load_arena(K.HostArena.from_payloads(small))
        res = gm.scan_packets(hits=True)
        check(res, hits_small, want_small)
        # mode 1 / kernel 1: EINVAL, the context stays usable
        for key, val in ((OPT_MODE, MODE_AUTOMATON), (OPT_KERNEL, KERNEL_GENERAL)):
            gm.set_option(key, val)
            assert g.kmpgpu_scan_packets(gm._ctx, None, None, None, None, None) == -2
            reset(gm)
        check(gm.scan_packets(hits=True), hits_small, want_small)
        # n_pkts == 0: zeros, nothing launched
        gm.load_arena(np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        res = gm.scan_packets(hits=True)
        assert res["pkt_counts"].tolist() == [0] * len(pats) and res["counts"].tolist() == [0] * len(pats)
        assert res["any"].size == 0 and res["hits"].shape == (len(pats), 0) and res["timing"].launches == 0
        # no patterns: ESTATE
        with GpuMatcher(0) as fresh:
            assert g.kmpgpu_scan_packets(fresh._ctx, None, None, None, None, None) == -3
    finally:
        reset(gm)


def test_arena_kept_in_place(gm, oracle):
    """OPT_REPACK = 0 with slots not back to back: the call packs the arena once, as kmpgpu_scan_offsets does."""
    rng = random.Random(7)
    payloads = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(0, 400))) for _ in range(500)]
    pats = [b"abc", b"ca", b"abcabca", b"b"]
    ln = np.array([len(t) for t in payloads], dtype=np.uint32)
    slot = np.maximum(16, (ln.astype(np.uint64) + 15) // 16 * 16) + 32           # gaps between the slots
    order = list(range(len(payloads)))
    rng.shuffle(order)                                                            # slots not in payload order
    off = np.zeros(len(payloads), dtype=np.uint64)
    pos = 0
    for k in order:
        off[k] = pos
        pos += int(slot[k])
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for k, t in enumerate(payloads):
        arena[int(off[k]):int(off[k]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    try:
        reset(gm)
        gm.set_option(OPT_REPACK, 0)
        gm.set_patterns(pats)
        gm.load_arena(arena, off, ln)
        want = MM.oracle_counts(oracle, payloads, pats)
        assert gm.scan()[0].tolist() == want
        check(gm.scan_packets(hits=True), MM.hits(MM.starts(payloads, pats)), want)
        assert gm.scan()[0].tolist() == want
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. 70 000 patterns on a few payloads (past the 16-bit pattern index)
# ------------------------------------------------------------------------------------------------
def test_many_patterns(gm, oracle):
    from test_gpu_limits import IDX16, _many_patterns, _text_payloads
    rng = random.Random(70000)
    payloads = _text_payloads(rng, 100, 300, b"abcd", extra=b"ef")
    pats, placed = _many_patterns(rng, payloads)
    assert len(pats) > 65536
    hits = MM.hits(MM.starts(payloads, pats))
    counts = [int(x) for x in oracle.count_payloads(payloads, pats, threads=8)]
    assert hits[IDX16 + 1:].any()
    try:
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        for name, kernel, fused in (KERNELS[0], KERNELS[2]):
            reset(gm)
            gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
            check(gm.scan_packets(hits=True), hits, counts)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. dense input: a match at every start offset
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True])
def test_dense(gm, oracle, uniform):
    rng = random.Random(16)
    m = 16
    lens = [1500] * 600 if uniform else [rng.randrange(0, 3000) for _ in range(3000)]
    payloads = [b"a" * L for L in lens]
    if not uniform:
        for k in range(0, len(payloads), 7):                 # a 0x00 cuts some payloads below the pattern's length
            t = bytearray(payloads[k])
            if t:
                t[rng.randrange(len(t))] = 0
                payloads[k] = bytes(t)
    pats = [b"a" * m]
    hits = np.array([[MM.text_end(t) >= m for t in payloads]])
    counts = [sum(max(0, MM.text_end(t) - m + 1) for t in payloads)]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        for name, kernel, fused in KERNELS:
            gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
            check(gm.scan_packets(hits=True), hits, counts)
        # and next to another dense pattern: the fused pass
        gm.set_option(OPT_KERNEL, KERNEL_AUTO); gm.set_option(OPT_FUSED, 1)
        pats2 = pats + [b"aa"]
        gm.set_patterns(pats2)
        hits2 = np.array([[MM.text_end(t) >= len(p) for t in payloads] for p in pats2])
        check(gm.scan_packets(hits=True), hits2, MM.oracle_counts(oracle, payloads, pats2))
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 7. full size: 1 M x 1500 B synthetic, the bench arena
# ------------------------------------------------------------------------------------------------
def test_full_size_1m(gm):
    needle = b"NEEDLE_16B_PATRN"
    sp = K.SynthParams.make(seed=1234, needle=needle, plant_permille=100)
    n, L, stride = 1_000_000, 1500, 1504
    d_arena = torch.empty(n * stride + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n, dtype=torch.int64, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        reset(gm)
        gm.set_stream(None)
        gm.fixed_index(d_off, d_len, L, 16)
        gm.synth_fill(d_arena, d_off, d_len, sp)
        gm.sync()
        planted = K.synth_count_planted(sp, n, L)
        gm.set_patterns([needle])
        gm.attach_arena(d_arena, d_off, d_len)
        res = gm.scan_packets(hits=True)
        assert int(res["pkt_counts"][0]) == int(res["any"].sum()) == planted == int(res["counts"][0])
        # the set of payloads: a host search over the host-side twin of the generator
        off, ln, nbytes = K.arena_layout(None, L, n)
        host = np.zeros(nbytes, dtype=np.uint8)
        K.synth_fill_host(host, off, ln, sp)
        want = np.zeros(n, dtype=bool)
        step = 10_000
        for k0 in range(0, n, step):
            buf = host[k0 * stride:(k0 + step) * stride].tobytes()
            want[k0:k0 + step] = [buf.find(needle, j * stride, j * stride + L) >= 0 for j in range(min(step, n - k0))]
        assert (off == np.arange(n, dtype=np.uint64) * stride).all()
        assert np.array_equal(res["any"], want) and np.array_equal(res["hits"][0], want)
    finally:
        reset(gm)
        del d_arena, d_off, d_len
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 8. the command lines: KMPGPU_PACKETS_FILE
# ------------------------------------------------------------------------------------------------
CLI_RUNS = [("serial", [], {}), ("openmp_data", ["3"], {}), ("serial", [], {"KMPGPU_RCCL": "1"}),
            ("openmp_data", ["3"], {"KMPGPU_DEVICE_EXTRACT": "1"}), ("serial", [], {"KMPGPU_NOCASE": "1"})]


@pytest.mark.parametrize("run", CLI_RUNS, ids=[f"{r[0]}-{i}" for i, r in enumerate(CLI_RUNS)])
def test_cli_packets_file(oracle, tokens, fixture_counts, tmp_path, run):
    prog, extra, env_extra = run
    nocase = env_extra.get("KMPGPU_NOCASE") == "1"
    arena = K.HostArena.from_pcap(os.path.join(DATA, "big_udp.pcap"), "udp")
    payloads = [arena.payload(k) for k in range(arena.n_pkts)]
    flags = [nocase] * len(tokens)
    hits = MM.hits(MM.starts(payloads, tokens, nocase=flags))
    want = sorted((int(k), int(i)) for i, k in np.argwhere(hits))
    counts = MM.oracle_counts(oracle, payloads, tokens, flags)
    if not nocase:
        assert counts == fixture_counts["fixtures"]["big_udp.pcap:udp"]["counts"]
    out = tmp_path / "packets.csv"
    r = run_cli(prog, "big_udp.pcap", extra=extra, env_extra=dict(env_extra, KMPGPU_PACKETS_FILE=str(out)), scrub=None)
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == K.format_report(tokens, counts)
    got = [tuple(int(x) for x in line.split(",")) for line in out.read_text().splitlines()]
    assert got == want                                # sorted by payload, then by pattern, as written
