"""Flow seams on the GPU (kmpgpu_load_seams, kmpgpu_seams_read, kmpgpu_scan_flows_seams; include/kmpgpu.h) against tests/seam_model.py, an
independent model written from the definitions.  Every comparison is exact: the arena byte for byte, index, metadata, records, and the
flow-space rule rows.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA

from gpu_support import (FLOW_A as A, FLOW_B as B, ONES, attach_slots, gm, load, meta_of_flows, reset, torch)  # noqa: F401  (gm: the context fixture)

import chain_model as CM
import flow_model as FM
import header_model as HM
import match_model as MM
import seam_model as SM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import HostArena
from multithreading_string_matching_amd.matcher import OPT_KERNEL, OPT_NONTEMPORAL, OPT_REPACK, OPT_WHOLE_PAYLOAD, SEAM_DTYPE, GpuMatcher

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
H = HM.header


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


@pytest.fixture(scope="module")
def sm():
    """the second context: the one that owns the seams"""
    m = GpuMatcher(0)
    yield m
    m.close()


def check_seams(dst, pay, meta, recs):
    """dst's arena, index, metadata and records against the model's, byte for byte"""
    seams = SM.payloads(pay, recs)
    want, off, ln = SM.arena(seams)
    got = dst.seams()
    assert got.dtype == SEAM_DTYPE and got.tobytes() == recs.tobytes(), [i for i in range(min(len(got), len(recs))) if got[i] != recs[i]][:4]
    assert dst.arena_info() == (len(seams), sum(len(s) for s in seams))
    if not len(seams):
        return seams
    a, o, l = dst.arena_download()
    assert np.array_equal(o, off) and np.array_equal(l, ln)
    assert len(a) >= len(want) and not a[len(want):].any()
    bad = np.flatnonzero(a[:len(want)] != want)
    assert bad.size == 0, [(int(b), int(np.searchsorted(off, b, side="right")) - 1) for b in bad[:8]]
    assert dst.meta().tobytes() == meta[recs["next"].astype(np.int64)].tobytes()
    return seams


# ------------------------------------------------------------------------------------------------
# 1. arena, index, metadata and records against the model
# ------------------------------------------------------------------------------------------------
def _capture(reach, seed, n=320, n_flows=40):
    """a few hundred payloads in about 40 flows with interleaved directions; lengths around 16 and around reach, so that tail_len and
    head_len take every residue mod 16 over the reaches"""
    rng = np.random.default_rng(seed)
    flow = np.concatenate([np.arange(n_flows), rng.integers(0, n_flows - 4, n - n_flows)])        # the last four flows: one payload each
    meta = meta_of_flows(flow, seed=seed)
    lens = rng.choice(sorted({0, 1, 15, 16, 17, max(reach - 1, 0), reach, reach + 1, 200} | set(range(2, 15)) | set(range(18, 34))), n)
    pay = [bytes(rng.integers(1, 256, int(x), dtype=np.uint8)) for x in lens]
    # a seam of 0 bytes: two empty payloads in a row in one direction of one flow
    fo = FM.flow_of(meta)
    pr = SM.pred(fo, SM.direction(meta, fo))
    k = int(np.flatnonzero(pr != SM.NONE)[5])
    pay[k] = pay[int(pr[k])] = b""
    return pay, meta


def _put(src, pay, meta, form):
    """the source loaded; attached with dirty slot padding; attached with gaps between the slots and kept in place.  Returns what must stay
    alive."""
    keep = None
    if form == "loaded":
        load(src, pay)
    elif form == "dirty":
        keep = attach_slots(src, pay, [t + b"\xAA" * (SM.slot(len(t)) - len(t)) for t in pay])
    else:
        src.set_option(OPT_REPACK, 0)
        keep = attach_slots(src, pay, [t + b"\xBB" * (SM.slot(len(t)) - len(t) + 16 * (k % 3)) for k, t in enumerate(pay)])
    src.set_meta(meta)
    return keep


@pytest.mark.parametrize("form", ["loaded", "dirty", "in_place"])
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("reach", [1, 15, 16, 98])
def test_arena_against_the_model(gm, sm, reach, directed, form):
    _arena_against_the_model(gm, sm, reach, directed, form)


def test_default_cache_policy(gm, sm):
    """OPT_NONTEMPORAL = 0 on the context that receives the seams: the other instantiation of the gather kernel"""
    _arena_against_the_model(gm, sm, 98, False, "loaded", seam_options=((OPT_NONTEMPORAL, 0),))


def _arena_against_the_model(gm, sm, reach, directed, form, seam_options=()):
    pay, meta = _capture(reach, seed=reach + 7 * directed)
    lens = [len(t) for t in pay]
    reset(gm, sm)
    try:
        for key, value in seam_options:
            sm.set_option(key, value)
        gm.set_patterns([b"x"])
        keep = _put(gm, pay, meta, form)
        gm.build_flows(directed)
        recs = SM.records(meta, lens, reach, directed)
        assert {int(t) % 16 for t in recs["tail_len"]} >= set(range(16) if reach >= 15 else range(2))
        assert sm.load_seams(gm, reach) == len(recs) > 200
        seams = check_seams(sm, pay, meta, recs)
        assert b"" in seams                                   # an empty seam owns a zero slot
        t = sm.last_timing()
        assert t.launches == 7 and t.kernel_ms > 0
        # read ranges
        n = len(recs)
        assert sm.seams(n, 0).size == 0 and sm.seams(3, 2).tobytes() == recs[3:5].tobytes()
        for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (ONES, 2)):
            with raises(EINVAL, "leave the"):
                sm.seams(first, count)
        assert sm._g.kmpgpu_seams_read(sm._ctx, None, 0, 1) == EINVAL
        del keep
    finally:
        reset(gm, sm)


def test_last_slot_of_a_borrowed_arena(gm, sm):
    """The arena ends with its last slot: the gather may read nothing behind it, and nothing in front of the first.  The tail of the
    last payload ends on the arena's last byte."""
    pay = [b"a" * 31, b"b" * 5, b"c" * 32]
    meta = meta_of_flows([0, 0, 0], seed=3)
    meta[:] = meta[0]
    ln = np.array([len(t) for t in pay], dtype=np.uint32)
    off = np.array([0, 32, 48], dtype=np.uint64)
    arena = np.frombuffer(pay[0] + b"\xCC" + pay[1] + b"\xCC" * 11 + pay[2], dtype=np.uint8).copy()
    assert len(arena) == 80
    keep = (torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    reset(gm, sm)
    gm.set_patterns([b"x"])
    gm.attach_arena(*keep)
    gm.set_meta(meta)
    gm.build_flows()
    for reach in (3, 17, 98):
        assert sm.load_seams(gm, reach) == 2
        check_seams(sm, pay, meta, SM.records(meta, ln, reach))
    del keep


# ------------------------------------------------------------------------------------------------
# 2. nothing depends on the run, and src is what it was
# ------------------------------------------------------------------------------------------------
def test_two_builds_are_byte_identical_and_src_is_untouched(gm, sm):
    pay, meta = _capture(98, seed=11)
    pats = [b"\x41", bytes([7, 9]), b"\x20\x20\x20"]
    reset(gm, sm)
    gm.set_patterns(pats)
    load(gm, pay)
    gm.set_meta(meta)
    gm.set_rules([([0], [1]), ([], [2])])
    gm.build_flows()

    def snapshot():
        out = []
        for res in (gm.scan_rules(hits=True), gm.scan_flows("rules", "flow", hits=True), gm.scan_flows("patterns", "packet", hits=True)):
            out.append((res["hits"].tobytes(), res["any"].tobytes(), res["counts"].tobytes(), res["timing"].launches))
        a, off, ln = gm.arena_download()
        out.append((a.tobytes(), off.tobytes(), ln.tobytes(), gm.meta().tobytes(), gm.flow_ids().tobytes(), gm.flows().tobytes()))
        return out

    before = snapshot()
    outs = []
    for _ in range(2):
        sm.load_seams(gm, 98)
        a, off, ln = sm.arena_download()
        outs.append((a.tobytes(), off.tobytes(), ln.tobytes(), sm.meta().tobytes(), sm.seams().tobytes()))
    assert outs[0] == outs[1]
    sm.set_patterns(pats)
    gm.scan_flow_seams(sm, hits=True)
    assert snapshot() == before


# ------------------------------------------------------------------------------------------------
# 3. the point of the feature
# ------------------------------------------------------------------------------------------------
X, Y, Z = (A, 40000, B, 80), (B, 80, A, 40000), (A + 1, 40001, B, 80)       # a client's segments, the server's answers, another connection


def _meta(rows):
    m = np.zeros(len(rows), dtype=HM.META_DTYPE)
    for k, (s, sp, d, dp) in enumerate(rows):
        m[k]["src_ip"], m[k]["src_port"], m[k]["dst_ip"], m[k]["dst_port"], m[k]["proto"] = s, sp, d, dp, 6
    return m


@pytest.mark.parametrize("case,rows,fires", [
    ("consecutive", [X, X, Z], [True, False]),
    ("across the two directions", [X, Y, Z], [False, False]),
    ("another flow's payload in between", [X, Z, X], [True, False]),
    ("the answer in between", [X, Y, X], [True]),
])
def test_split_content(gm, sm, case, rows, fires):
    pay = [b"GET /index.html HTTP/1.1"] * len(rows)
    k2 = max(k for k, r in enumerate(rows) if r != Z and k > 0)          # where the content's second half travels
    pay[0], pay[k2] = b"GET /adm", b"in HTTP/1.1"
    meta = _meta(rows)
    pats = [b"/admin", b"intranet"]
    rules = [([0], [1])]
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns(pats)
    load(gm, pay)
    gm.set_meta(meta)
    gm.set_rules(rules)
    n_flows = gm.build_flows()
    assert n_flows == len(fires)
    assert not gm.scan_flows("rules", "flow", hits=True)["hits"].any()          # /admin hits in neither payload
    sm.load_seams(gm)
    res = gm.scan_flow_seams(sm, hits=True)
    assert res["hits"].tolist() == [fires], case
    assert res["flow_counts"].tolist() == [sum(fires)] and res["any"].tolist() == fires
    assert res["counts"].tolist() == [0, 0]                  # cross-boundary matches are not counted
    # the model says the same
    fo = FM.flow_of(meta)
    recs = SM.records(meta, [len(t) for t in pay], 98)
    seam_hits = MM.hits(MM.starts(SM.payloads(pay, recs), pats), 2)
    want = SM.flow_rules(MM.hits(MM.starts(pay, pats), 2), seam_hits, fo, fo[recs["next"].astype(np.int64)], rules, n_flows)
    assert want.tolist() == [fires]


# ------------------------------------------------------------------------------------------------
# 4. the combined rows against the model
# ------------------------------------------------------------------------------------------------
def _world(seed, n=260, n_flows=30):
    """Every flow direction's stream is written first -- text over four letters with the patterns planted --, then cut into payloads at random
    places, so that patterns of every length straddle boundaries; a 0x00 is put near some of the cuts."""
    rng = np.random.default_rng(seed)
    lens_pat = [1, 2, 3, 4, 5, 8, 15, 16, 17, 33, 64, 98, 99]
    pats = [bytes(rng.choice([0x41, 0x62, 0x43, 0x64], m).astype(np.uint8)) for m in lens_pat]
    flow = np.concatenate([np.arange(n_flows), rng.integers(0, n_flows - 3, n - n_flows)])
    meta = meta_of_flows(flow, seed=seed)
    fo = FM.flow_of(meta)
    dr = SM.direction(meta, fo)
    pay = [b""] * n
    for chain in sorted({(int(f), int(d)) for f, d in zip(fo, dr)}):
        ks = [k for k in range(n) if (int(fo[k]), int(dr[k])) == chain]
        stream = bytearray()
        for _ in range(2 + len(ks)):
            stream += bytes(rng.choice([0x61, 0x62, 0x63, 0x64], int(rng.integers(0, 60))).astype(np.uint8))
            if rng.integers(0, 3):
                p = pats[int(rng.integers(len(pats)))]
                stream += p if rng.integers(0, 2) else p.swapcase()
        cuts = np.sort(rng.integers(0, len(stream) + 1, len(ks) - 1)).tolist()
        for c in cuts:
            if rng.integers(0, 5) == 0 and len(stream):
                stream[min(max(c + int(rng.integers(-6, 6)), 0), len(stream) - 1)] = 0
        for k, (lo, hi) in zip(ks, zip([0] + cuts, cuts + [len(stream)])):
            pay[k] = bytes(stream[lo:hi])
    return pats, pay, meta, fo


@pytest.mark.parametrize("whole_seams", [0, 1])
@pytest.mark.parametrize("whole", [0, 1])
@pytest.mark.parametrize("nocase", [False, True])
def test_combined_rows_against_the_model(gm, sm, oracle, nocase, whole, whole_seams):
    pats, pay, meta, fo = _world(seed=21 + nocase)
    n_pat, n_flows = len(pats), int(fo.max()) + 1
    nc = [bool(nocase and i % 2 == 0) for i in range(n_pat)]
    chains = [(1, (2, 0, 40))]
    heads = [H(proto=17, sport=(1000, 1002))]
    reach = 98
    lens = [len(t) for t in pay]
    reset(gm, sm)
    try:
        for m in (gm, sm):
            m.set_patterns(pats, nocase=nc)
        gm.set_option(OPT_WHOLE_PAYLOAD, whole)
        sm.set_option(OPT_WHOLE_PAYLOAD, whole_seams)
        load(gm, pay)
        gm.set_meta(meta)
        gm.set_chains(chains)
        gm.set_headers(heads)
        c0, h0 = gm.chain(0), gm.hdr(0)
        rng = np.random.default_rng(5)
        rules = [([i], []) for i in range(n_pat)] + [([c0], []), ([h0], []), ([0, c0], [h0]), ([], [12, 11])]
        for _ in range(12):
            terms = rng.permutation(n_pat + 2)[: int(rng.integers(1, 5))].tolist()
            cut = int(rng.integers(0, len(terms) + 1))
            rules.append((terms[:cut], terms[cut:]))
        gm.set_rules(rules)
        assert gm.build_flows() == n_flows
        recs = SM.records(meta, lens, reach)
        assert sm.load_seams(gm, reach) == len(recs)
        seams = check_seams(sm, pay, meta, recs)
        st = MM.starts(pay, pats, nocase=nc, whole=bool(whole))
        src_terms = np.concatenate([MM.hits(st, n_pat), CM.chain_rows(st, pats, chains), HM.header_rows(meta, lens, heads)])
        seam_hits = MM.hits(MM.starts(seams, pats, nocase=nc, whole=bool(whole_seams)), n_pat)
        seam_flow = fo[recs["next"].astype(np.int64)]
        want = SM.flow_rules(src_terms, seam_hits, fo, seam_flow, rules, n_flows)
        plain = FM.flow_rules(src_terms, fo, rules, n_flows)
        # the seams matter here: long patterns are found across boundaries only, and a negated term bars flows it did not bar
        assert (want[:n_pat] & ~plain[:n_pat]).sum() > 10 and (want[9:n_pat] & ~plain[9:n_pat]).any() and (plain & ~want).any()
        res = gm.scan_flow_seams(sm, hits=True)
        bad = np.argwhere(res["hits"] != want)
        assert bad.size == 0, [(int(r), int(f), bool(want[r, f])) for r, f in bad[:8]]
        assert res["flow_counts"].tolist() == want.sum(axis=1).tolist() and res["any"].tolist() == want.any(axis=0).tolist()
        assert res["counts"].tolist() == MM.oracle_counts(oracle, pay, pats, nc, bool(whole))        # what kmpgpu_scan(src) returns
        base = gm.scan_flows("rules", "flow", hits=True)
        assert np.array_equal(base["hits"], plain)
        assert res["timing"].launches == base["timing"].launches + sm.scan_packets()["timing"].launches + 1
        # the raw words: the bits at n_flows and above are 0
        Wf = (n_flows + 63) // 64
        hit_w, any_w = np.full((len(rules), Wf), ONES, dtype=np.uint64), np.full(Wf, ONES, dtype=np.uint64)
        _lib.gpu_check(gm._g.kmpgpu_scan_flows_seams(gm._ctx, sm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_flows_seams")
        assert np.array_equal(hit_w, MM.words(want)) and np.array_equal(any_w, MM.words(want.any(axis=0)))
        if whole and whole_seams:
            # whole payloads on both: a seam hit is a match of the concatenated stream (tests/test_seam_model.py), so a pattern row of the
            # combined terms says "the flow direction's stream or one of its payloads holds the pattern"
            dr = SM.direction(meta, fo)
            for i in (9, 12):
                for f in range(n_flows):
                    streams = [b"".join(pay[k] for k in range(len(pay)) if fo[k] == f and dr[k] == d) for d in (0, 1)]
                    held = any((MM.fold(s) if nc[i] else s).find(MM.fold(pats[i]) if nc[i] else pats[i]) >= 0 for s in streams)
                    assert bool(want[i, f]) <= held
    finally:
        reset(gm, sm)


def test_windows_and_options_of_the_seam_context_are_its_own(gm, sm):
    """A seam is a payload of its own: dst's windows count from the seam's first byte."""
    pay = [b"....GET /adm", b"in HTTP/1.1"]
    meta = _meta([X, X])
    pats = [b"/admin"]
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns(pats)
    load(gm, pay)
    gm.set_meta(meta)
    gm.set_rules([([0], [])])
    gm.build_flows()
    sm.load_seams(gm, 8)                                     # the seam: b"GET /admin HTTP/" -- /admin at offset 4
    assert SM.payloads(pay, SM.records(meta, [12, 11], 8)) == [b"GET /admin HTTP/"]
    for window, fires in (((0, 3), False), ((4, 4), True), ((5, None), False)):
        sm.set_windows([window])
        assert gm.scan_flow_seams(sm, hits=True)["hits"].tolist() == [[fires]]
    sm.set_windows([(0, None)])
    sm.load_seams(gm, 4)                                     # reach + 1 = 5 < 6: the seam b"/admin H" still holds it; reach 2 does not
    assert gm.scan_flow_seams(sm, hits=True)["hits"].tolist() == [[True]]
    sm.load_seams(gm, 2)
    assert gm.scan_flow_seams(sm, hits=True)["hits"].tolist() == [[False]]


# ------------------------------------------------------------------------------------------------
# 5. past the grid sizes: 300 000 payloads are past the 262 144 of the per-payload kernels' grids, past one scan tile, and enough for the
#    sort to leave its single-block path
# ------------------------------------------------------------------------------------------------
N_BIG = 300_000


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(77)
    lens = rng.integers(16, 49, N_BIG).astype(np.uint32)
    size = ((lens + 15) // 16 * 16).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64)
    arena = rng.integers(1, 256, int(size.sum()) + 64, dtype=np.uint8)
    arena[-64:] = 0
    ends = (off + lens).astype(np.int64)
    for d in range(15):                                       # 0x00 behind every payload's end
        at = ends + d
        arena[at[at < (off + size).astype(np.int64)]] = 0
    return arena, off, lens


@pytest.mark.parametrize("shape", ["many", "one", "each", "two"])
def test_past_the_grid_sizes(gm, sm, big, shape):
    arena, off, lens = big
    k = np.arange(N_BIG)
    flow = {"many": (k * 2654435761 >> 7) % 5000, "one": np.zeros(N_BIG, dtype=np.int64), "each": k, "two": k % 2}[shape]
    meta = meta_of_flows(flow, seed=4)                         # (a flow is an address of its own)
    reach = 20
    pats = [b"\x41\x42"]
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns(pats)
    gm.load_arena(arena, off, lens)
    gm.set_meta(meta)
    gm.set_rules([([0], [])])
    n_flows = gm.build_flows()
    recs = SM.records_np(meta, lens, reach)
    assert sm.load_seams(gm, reach) == len(recs)
    assert len(recs) == {"one": N_BIG - 2, "each": 0, "two": N_BIG - 4}.get(shape, len(recs)) and (shape == "each" or len(recs) > 250_000)
    got = sm.seams()
    assert got.tobytes() == recs.tobytes(), np.flatnonzero(got != recs)[:4]
    if shape == "each":
        assert sm.arena_info() == (0, 0)
        res, base = gm.scan_flow_seams(sm, hits=True), gm.scan_flows("rules", "flow", hits=True)
        assert np.array_equal(res["hits"], base["hits"]) and res["timing"].launches == base["timing"].launches
        return
    # the arena, from the source's bytes by numpy: byte b of seam j
    prev, nxt = recs["prev"].astype(np.int64), recs["next"].astype(np.int64)
    tl, hl = recs["tail_len"].astype(np.int64), recs["head_len"].astype(np.int64)
    sl = tl + hl
    size = np.maximum(16, (sl + 15) // 16 * 16)
    soff = np.concatenate([[0], np.cumsum(size)[:-1]])
    want = np.zeros(int(size.sum()), dtype=np.uint8)
    for b in range(2 * reach):
        in_tail, in_head = b < tl, (b >= tl) & (b < sl)
        want[(soff + b)[in_tail]] = arena[(off.astype(np.int64)[prev] + lens.astype(np.int64)[prev] - tl + b)[in_tail]]
        want[(soff + b)[in_head]] = arena[(off.astype(np.int64)[nxt] + b - tl)[in_head]]
    a, o, l = sm.arena_download()
    assert np.array_equal(o, soff.astype(np.uint64)) and np.array_equal(l, sl.astype(np.uint32))
    assert not a[len(want):].any() and np.array_equal(a[:len(want)], want)
    assert sm.meta().tobytes() == meta[nxt].tobytes()
    if shape in ("many", "two"):
        # the combined rows: the two-byte pattern per payload and per seam, by numpy
        def holds(buf, o_, l_):
            at = np.flatnonzero((buf[:-1] == 0x41) & (buf[1:] == 0x42))
            j = np.searchsorted(o_, at, side="right") - 1
            ok = at + 2 <= (o_ + l_)[j]
            out = np.zeros(len(o_), dtype=bool)
            out[j[ok]] = True
            return out
        fo = FM.flow_of_np(meta)
        src_hit, seam_hit = holds(arena, off.astype(np.int64), lens.astype(np.int64)), holds(want, soff, sl)
        want_rows = SM.flow_rules(src_hit[None, :], seam_hit[None, :], fo, fo[nxt], [([0], [])], n_flows)
        res = gm.scan_flow_seams(sm, hits=True)
        assert np.array_equal(res["hits"], want_rows)
        assert shape == "two" or (want_rows & ~FM.flow_rules(src_hit[None, :], fo, [([0], [])], n_flows)).any()


# ------------------------------------------------------------------------------------------------
# 6. errors and state transitions
# ------------------------------------------------------------------------------------------------
def _no_seams(m, src):
    with raises(ESTATE, "kmpgpu_seams_read: no seams"):
        m.seams()
    with raises(ESTATE, "kmpgpu_scan_flows_seams: no seams"):
        src.scan_flow_seams(m)


def test_errors_and_state(gm, sm):
    pay, meta = _capture(16, seed=2)
    lens = [len(t) for t in pay]
    pats = [b"ab", b"c"]
    G = gm._g
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns(pats)
    load(gm, pay)
    load(sm, [b"kept"])
    n = C.c_uint64(99)

    def kept():
        a, off, ln = sm.arena_download()
        return sm.arena_info() == (1, 4) and bytes(a[:4]) == b"kept"

    # src without built flows
    with raises(ESTATE, "kmpgpu_load_seams: no flows"):
        sm.load_seams(gm)
    gm.set_meta(meta)
    with raises(ESTATE, "kmpgpu_load_seams: no flows"):
        sm.load_seams(gm)
    gm.set_rules([([0], [1])])
    gm.build_flows()
    # the arguments
    assert G.kmpgpu_load_seams(sm._ctx, sm._ctx, 16, C.byref(n)) == EINVAL and b"kmpgpu_load_seams: dst and src are the same" in G.kmpgpu_last_error()
    assert n.value == 0
    assert G.kmpgpu_load_seams(None, gm._ctx, 16, None) == EINVAL and G.kmpgpu_load_seams(sm._ctx, None, 16, None) == EINVAL
    assert b"kmpgpu_load_seams: ctx is NULL" in G.kmpgpu_last_error()
    for reach in (0, 99, 1 << 31):
        with raises(EINVAL, "kmpgpu_load_seams: reach"):
            sm.load_seams(gm, reach)
    if torch.cuda.device_count() > 1:
        with GpuMatcher(1) as far:
            with raises(EINVAL, "kmpgpu_load_seams: the contexts sit on devices"):
                far.load_seams(gm)
    assert kept()
    _no_seams(sm, gm)
    # either context between kmpgpu_load_frames_begin and _finish
    fr = _lib.Frames()
    err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
    assert _lib.host_lib().kmp_frames_from_pcap(os.path.join(DATA, "udp_1000.pcap").encode(), None, None, C.byref(fr), err) == 0
    try:
        with GpuMatcher(0) as other:
            other.set_patterns(pats)
            assert G.kmpgpu_load_frames_begin(other._ctx, fr.bytes, fr.nbytes, fr.off, fr.caplen, fr.n, 0) == 0
            with raises(ESTATE, "kmpgpu_load_seams: dst sits between kmpgpu_load_frames_begin"):
                other.load_seams(gm)
            assert G.kmpgpu_load_seams(sm._ctx, other._ctx, 16, None) == ESTATE and b"src sits between" in G.kmpgpu_last_error()
            assert G.kmpgpu_load_frames_finish(other._ctx, C.byref(n)) == 0
    finally:
        _lib.host_lib().kmp_frames_free(C.byref(fr))
    assert kept()
    # a list; what scan_flows_seams asks of the two contexts
    recs = SM.records(meta, lens, 16)
    assert sm.load_seams(gm, 16) == len(recs)
    check_seams(sm, pay, meta, recs)
    want = gm.scan_flow_seams(sm, hits=True)["hits"]
    assert G.kmpgpu_scan_flows_seams(None, sm._ctx, None, None, None, None, None) == EINVAL
    assert G.kmpgpu_scan_flows_seams(gm._ctx, None, None, None, None, None, None) == EINVAL
    assert G.kmpgpu_scan_flows_seams(gm._ctx, gm._ctx, None, None, None, None, None) == EINVAL
    sm.set_patterns([b"ab", b"d"])
    with raises(ESTATE, "kmpgpu_scan_flows_seams: the contexts do not hold the same patterns"):
        gm.scan_flow_seams(sm)
    sm.set_patterns(pats, nocase=[True, False])               # the same bytes, other flags
    with raises(ESTATE, "do not hold the same patterns"):
        gm.scan_flow_seams(sm)
    sm.set_patterns(pats[:1])
    with raises(ESTATE, "do not hold the same patterns"):
        gm.scan_flow_seams(sm)
    sm.set_patterns(pats)                                     # (set_patterns keeps the arena and the list)
    assert np.array_equal(gm.scan_flow_seams(sm, hits=True)["hits"], want)
    # everything else as kmpgpu_scan_flows on src and as kmpgpu_scan_packets on seams
    gm.set_rules([])
    with raises(ESTATE, "kmpgpu_scan_flows_seams: no rules set"):
        gm.scan_flow_seams(sm)
    gm.set_rules([([0], [1])])
    for m in (gm, sm):
        m.set_option(OPT_KERNEL, 1)
        with raises(EINVAL, "kmpgpu_scan_flows_seams runs on the streaming kernels only"):
            gm.scan_flow_seams(sm)
        m.set_option(OPT_KERNEL, 0)
    # a list of another generation of src's flows, or of another context's
    gm.build_flows()
    with raises(ESTATE, "kmpgpu_scan_flows_seams: the seam list was not built from src's current flows"):
        gm.scan_flow_seams(sm)
    assert sm.seams().tobytes() == recs.tobytes()             # the list itself stays
    sm.load_seams(gm, 16)
    assert np.array_equal(gm.scan_flow_seams(sm, hits=True)["hits"], want)
    gm.set_meta(meta)                                         # drops src's flows
    with raises(ESTATE, "kmpgpu_scan_flows_seams: no flows"):
        gm.scan_flow_seams(sm)
    gm.build_flows()
    with raises(ESTATE, "not built from src's current flows"):
        gm.scan_flow_seams(sm)
    with GpuMatcher(0) as other:
        other.set_patterns(pats)
        load(other, pay)
        other.set_meta(meta)
        other.set_rules([([0], [1])])
        other.build_flows()
        sm.load_seams(other, 16)
        assert np.array_equal(other.scan_flow_seams(sm, hits=True)["hits"], want)
        with raises(ESTATE, "not built from src's current flows"):
            gm.scan_flow_seams(sm)
    # whatever replaces dst's arena drops the seam state
    sm.load_seams(gm, 16)
    for replace in (lambda: load(sm, [b"kept"]), lambda: sm.load_selected(gm, np.ones(len(pay), dtype=bool)),
                    lambda: sm.load_arena(HostArena.from_payloads([]))):
        assert sm.seams().tobytes() == recs.tobytes()
        replace()
        _no_seams(sm, gm)
        sm.load_seams(gm, 16)
    keep = attach_slots(sm, [b"kept"], [b"kept" + b"\0" * 12])
    _no_seams(sm, gm)
    del keep
    # dst as the source of another list: a context cannot be both
    sm.load_seams(gm, 16)
    with raises(ESTATE, "kmpgpu_load_seams: no flows"):
        gm.load_seams(sm, 16)
    assert np.array_equal(gm.scan_flow_seams(sm, hits=True)["hits"], want)


# ------------------------------------------------------------------------------------------------
# 7. an empty seam list
# ------------------------------------------------------------------------------------------------
def test_empty_seam_list_equals_scan_flows(gm, sm):
    pay = [b"GET /adm", b"in HTTP", b"/admin", b"-"]
    meta = _meta([X, Y, Z, (A + 2, 1, B, 2)])                # every flow direction a single payload
    pats = [b"/admin", b"GET"]
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns(pats)
    load(gm, pay)
    load(sm, [b"/admin GET"])
    gm.set_meta(meta)
    gm.set_rules([([0], []), ([1], [0]), ([], [0, 1])])
    assert gm.build_flows() == 3
    n = C.c_uint64(99)
    assert gm._g.kmpgpu_load_seams(sm._ctx, gm._ctx, 98, C.byref(n)) == 0 and n.value == 0
    assert sm.arena_info() == (0, 0)
    load(sm, [b"/admin GET"])
    assert sm.load_seams(gm) == 0
    assert sm.arena_info() == (0, 0) and sm.seams().size == 0 and sm.last_timing().launches == 5
    with raises(EINVAL, "leave the"):
        sm.seams(0, 1)
    base, res = gm.scan_flows("rules", "flow", hits=True), gm.scan_flow_seams(sm, hits=True)
    for key in ("hits", "any", "flow_counts", "counts"):
        assert np.array_equal(res[key], base[key]), key
    assert res["timing"].launches == base["timing"].launches
    # no payloads at all
    gm.load_arena(HostArena.from_payloads([]))
    assert gm.build_flows() == 0
    load(sm, [b"/admin GET"])
    assert sm.load_seams(gm) == 0 and sm.arena_info() == (0, 0) and sm.seams().size == 0 and sm.last_timing().launches == 0
    res = gm.scan_flow_seams(sm, hits=True)
    assert res["flow_counts"].tolist() == [0, 0, 0] and res["hits"].shape == (3, 0) and res["timing"].launches == 0
