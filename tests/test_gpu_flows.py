"""Flows on the GPU (kmpgpu_flows_build, kmpgpu_flows_read, kmpgpu_flow_ids_read, kmpgpu_scan_flows, kmpgpu_flows_select; include/kmpgpu.h)
against tests/flow_model.py, an independent model written from the definitions with a Python dict keyed by the tuple.  Every comparison
is exact: ids, records, folded rows, expanded bitmaps.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA

from gpu_support import (FLOW_A as A, FLOW_B as B, KERNELS, ONES, attach_slots, check_fold as _check_fold, gm, load,  # noqa: F401  (gm: the context fixture)
                         meta_of_flows as _meta_of_flows, reset, run_cli, strip_elapsed, torch)

import chain_model as CM
import flow_model as FM
import header_model as HM
import match_model as MM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import HostArena
from multithreading_string_matching_amd.matcher import (FLOW_DTYPE, OPT_FLOW_SLOTS, OPT_FUSED, OPT_KEEP_META, OPT_KERNEL, OPT_REPACK,
                                                        OPT_WHOLE_PAYLOAD, GpuMatcher)
from test_flow_model import FIXTURES

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
TILE = 256 * 4                # KMP_SCAN_TILE
SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
SHAPE_PATS = [b"GET", b"zz"]
H = HM.header


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


def _check_build(m, meta, lens, directed=False, n_flows=None):
    got = m.build_flows(directed)
    fo, recs = FM.flow_of(meta, directed), FM.records(meta, lens, directed)
    assert got == len(recs) and (n_flows is None or got == n_flows)
    ids = m.flow_ids()
    assert ids.dtype == np.uint32 and np.array_equal(ids, fo), np.flatnonzero(ids != fo)[:8]
    r = m.flows()
    assert r.dtype == FLOW_DTYPE and r.tobytes() == recs.tobytes(), [i for i in range(len(recs)) if r[i] != recs[i]][:4]
    return fo, recs


# ------------------------------------------------------------------------------------------------
# 1. payload counts x flow shapes: ids, records, and the pattern family folded
# ------------------------------------------------------------------------------------------------
def _shapes(n):
    k = np.arange(n)
    shapes = {"one": np.zeros(n, dtype=np.int64), "each": k, "two": k % 2, "runs": (k + 32) // 64}
    for f in (63, 64, 65, 128, 129):
        shapes[f"f{f}"] = k % f
    return shapes


@pytest.mark.parametrize("n", SIZES)
def test_shapes(gm, n):
    # a payload holds GET where its index is a multiple of 3, and none holds zz but the last one
    payloads = [(b"GET /%d" % k if k % 3 == 0 else b"get /%d" % k) + (b" zz" if k == n - 1 else b"") for k in range(n)]
    hits = MM.hits(MM.starts(payloads, SHAPE_PATS), len(SHAPE_PATS))
    assert hits[0].sum() == (n + 2) // 3 and hits[1].tolist() == [False] * (n - 1) + [True]
    lens = [len(t) for t in payloads]
    reset(gm)
    gm.set_patterns(SHAPE_PATS)
    load(gm, payloads)
    for name, flow in _shapes(n).items():
        meta = _meta_of_flows(flow, seed=n)
        gm.set_meta(meta)
        fo, recs = _check_build(gm, meta, lens, n_flows=len(set(flow.tolist())))
        assert np.array_equal(fo, flow), name             # (the shapes number their flows in the order of their first payload)
        _check_fold(gm, "patterns", "packet", FM.fold(hits, fo))
        if name in ("two", "f65"):
            _check_build(gm, meta, lens, directed=True)


# ------------------------------------------------------------------------------------------------
# 2. the key
# ------------------------------------------------------------------------------------------------
def test_the_key(gm):
    base = (A, B, 1000, 80, 6)
    one_field = [(A + 1, B, 1000, 80, 6), (A, B + 1, 1000, 80, 6), (A, B, 1001, 80, 6), (A, B, 1000, 81, 6), (A, B, 1000, 80, 17)]
    cases = [
        ([base] + one_field + [base], [0, 1, 2, 3, 4, 5, 0], [0, 1, 2, 3, 4, 5, 0]),          # keys that differ in exactly one field
        ([base, (B, A, 80, 1000, 6), base], [0, 0, 0], [0, 1, 0]),                                # the two directions of one conversation
        ([(A, B, 1, 2, 17), (A, B, 2, 1, 17), (B, A, 2, 1, 17), (B, A, 1, 2, 17)], [0, 1, 0, 1], [0, 1, 2, 3]),      # A:1 -> B:2 against A:2 -> B:1
        ([(A, A, 1, 2, 17), (A, A, 2, 1, 17)], [0, 0], [0, 1]),                                   # src == dst, swapped ports
        ([(0, 0, 0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 65535, 65535, 255), (0, 0xFFFFFFFF, 0, 65535, 0)], [0, 1, 2], [0, 1, 2]),
    ]
    reset(gm)
    gm.set_patterns(SHAPE_PATS)
    for recs, want, want_directed in cases:
        meta = HM.meta_array(recs)
        load(gm, [b"x"] * len(recs))
        gm.set_meta(meta)
        for directed, w in ((False, want), (True, want_directed)):
            fo, _ = _check_build(gm, meta, [1] * len(recs), directed)
            assert fo.tolist() == w
    # records that differ only in `reserved` are one flow, and `first` is the first payload's record as it is
    meta = HM.meta_array([base, base, base])
    meta["reserved"][0] = (7, 0, 0)
    meta["reserved"][2] = (0, 0, 9)
    load(gm, [b"x"] * 3)
    gm.set_meta(meta)
    fo, recs = _check_build(gm, meta, [1] * 3)
    assert fo.tolist() == [0, 0, 0] and gm.flows()["first"].tobytes() == meta[:1].tobytes()


# ------------------------------------------------------------------------------------------------
# 3. KMPGPU_OPT_FLOW_SLOTS, and nothing depends on the run
# ------------------------------------------------------------------------------------------------
def _tight(n_flows, slots):
    """n_flows distinct random keys, then as many of them again as the table leaves room for"""
    rng = np.random.default_rng(n_flows)
    keys = [(int(rng.integers(1 << 32)), int(rng.integers(1 << 32)), int(rng.integers(1 << 16)), int(rng.integers(1 << 16)), 17) for _ in range(n_flows)]
    again = rng.permutation(n_flows)[: slots - 1 - n_flows]
    meta = HM.meta_array(keys + [keys[int(i)] for i in again])
    payloads = [b"GET" if i % 5 == 0 else b"zz" if i % 7 == 0 else b"-" for i in range(len(meta))]
    return meta, payloads


@pytest.mark.parametrize("n_flows,slots", [(1000, 1024), (257, 512)])
def test_flow_slots(gm, n_flows, slots):
    meta, payloads = _tight(n_flows, slots)
    n = len(meta)
    assert n_flows < n < slots
    lens = [len(t) for t in payloads]
    hits = MM.hits(MM.starts(payloads, SHAPE_PATS), 2)
    reset(gm)
    try:
        gm.set_patterns(SHAPE_PATS)
        load(gm, payloads)
        gm.set_meta(meta)
        outs = []
        for value in (slots, 0, slots, slots):           # nearly full, auto, and nearly full twice more: byte-identical
            gm.set_option(OPT_FLOW_SLOTS, value)
            fo, _ = _check_build(gm, meta, lens, n_flows=n_flows)
            res = _check_fold(gm, "patterns", "packet", FM.fold(hits, fo))
            outs.append((gm.flow_ids().tobytes(), gm.flows().tobytes(), res["hits"].tobytes()))
        assert all(o == outs[0] for o in outs)
        # a value that is not above the payload count, or no power of two: the build refuses, and the flows before it are kept or gone
        # but never half built
        for bad in (n, slots // 2, slots + 1, 3 * slots // 2):
            gm.set_option(OPT_FLOW_SLOTS, bad)
            with raises(EINVAL, "KMPGPU_OPT_FLOW_SLOTS"):
                gm.build_flows()
        with raises(EINVAL, "flow slots"):
            gm.set_option(OPT_FLOW_SLOTS, -1)
    finally:
        gm.set_option(OPT_FLOW_SLOTS, 0)


def test_three_builds_of_a_capture_are_byte_identical(gm):
    host = HostArena.from_pcap(os.path.join(DATA, "big_udp.pcap"), "udp", with_meta=True)
    reset(gm)
    gm.set_patterns([b"a", b"the", b"HTTP"])
    gm.load_arena(host)
    outs = []
    for _ in range(3):
        n = gm.build_flows()
        outs.append((n, gm.flow_ids().tobytes(), gm.flows().tobytes(), gm.scan_flows("patterns", hits=True)["hits"].tobytes()))
    assert outs[0][0] == FIXTURES[("big_udp.pcap", "udp")][2] and outs[1] == outs[0] and outs[2] == outs[0]


# ------------------------------------------------------------------------------------------------
# 4. the committed captures, by both routes to the metadata
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcap,mode", [("big_udp.pcap", "udp"), ("very_big_udp.pcap", "udp"), ("udp_1000.pcap", "udp"), ("udp_1000.pcap", "tcp"),
                                       ("tcp.pcap", "tcp")])
def test_fixtures(gm, pcap, mode):
    path = os.path.join(DATA, pcap)
    n, n_dir, n_bi, _ = FIXTURES[(pcap, mode)]
    host = HostArena.from_pcap(path, mode, with_meta=True)
    assert host.n_pkts == n
    lens = host.len.tolist()
    reset(gm)
    try:
        gm.set_patterns(SHAPE_PATS)
        gm.load_arena(host)
        _check_build(gm, host.meta, lens, False, n_bi)
        _check_build(gm, host.meta, lens, True, n_dir)
        gm.set_option(OPT_KEEP_META, 1)
        assert gm.load_pcap_frames(path, mode)[0] == n
        with raises(ESTATE, "no flows"):                  # the load dropped them
            gm.flows()
        _check_build(gm, host.meta, lens, True, n_dir)
        _check_build(gm, host.meta, lens, False, n_bi)
    finally:
        gm.set_option(OPT_KEEP_META, 0)


# ------------------------------------------------------------------------------------------------
# 5. the fold of every family, and rules per flow
# ------------------------------------------------------------------------------------------------
PATS = [b"GET", b"/admin", b"xyz", b"ALL", b"NONE!", b"LAST", b"EVRY"]
RELATIONS = [(0, 1, 0, 8), (3, 6, None, None), (4, 0, None, None), (5, 3, None, None)]            # planted, everywhere, nowhere, the last payload
CHAINS = [(0, (1, 0, 4)), (3, (6, None, None)), (4, (0, None, None)), (5, (3, None, None)), (0, (1, 0, 8), (2, 0, None))]
HEADS = [H(proto=17, sport=(1000, 1003)), H(src=(B, 0xFFFFFFFF))]


@pytest.fixture(scope="module")
def world():
    """about 300 payloads in 40 flows, every row family over them, and the model's rows"""
    n, n_flows = 301, 40
    rng = np.random.default_rng(5)
    p = 1.0 / (np.arange(n_flows) + 1.0) ** 1.2           # a few big flows and many of one or two payloads
    flow = np.concatenate([np.arange(n_flows), rng.choice(n_flows, n - n_flows, p=p / p.sum())])
    meta = _meta_of_flows(flow, seed=9)
    bodies = [b"GET /admin xyz", b"GET  /admin", b"xyz only", b"get /ADMIN", b"/admin GET", b"nothing", b"GET /adminxyz", b""]
    payloads = [b"ALL " + bodies[int(rng.integers(len(bodies)))] + b" EVRY" for _ in range(n)]
    payloads[n - 1] = b"ALL EVRY LAST"
    st = MM.starts(payloads, PATS)
    hits = MM.hits(st, len(PATS))
    rel, ch = MM.relation_rows(st, PATS, RELATIONS), CM.chain_rows(st, PATS, CHAINS)
    hdr = HM.header_rows(meta, [len(t) for t in payloads], HEADS)
    last = [False] * (n - 1) + [True]
    for rows, every, nowhere, at_last in ((hits, 3, 4, 5), (rel, 1, 2, 3), (ch, 1, 2, 3)):
        assert rows[every].all() and not rows[nowhere].any() and rows[at_last].tolist() == last
        assert 0 < rows[0].sum() < n
    assert 0 < hdr[0].sum() < n and 0 < hdr[1].sum() < n
    fo = FM.flow_of(meta)
    assert int(fo.max()) + 1 == n_flows and np.array_equal(fo, flow)
    return payloads, meta, fo, hits, rel, ch, hdr


def _setup(m, world, kernel=None, fused=None):
    payloads, meta = world[0], world[1]
    reset(m)
    if kernel is not None:
        m.set_option(OPT_KERNEL, kernel)
        m.set_option(OPT_FUSED, fused)
    m.set_patterns(PATS)
    load(m, payloads)
    m.set_meta(meta)
    m.set_relations(RELATIONS)
    m.set_chains(CHAINS)
    m.set_headers(HEADS)


def _rules(m):
    np_, r0, c0, h0 = len(PATS), m.rel(0), m.chain(0), m.hdr(0)
    return [([0, 1], []), ([3], []), ([4], []), ([5], []), ([], [4]), ([], [3]), ([0, r0], [2]), ([c0 + 4, h0], []), ([2], [h0 + 1, r0 + 3]),
            ([], [0, c0, h0 + 1]), ([r0 + 1, c0 + 1, 6, 3, h0], [4, 5])]


@pytest.mark.parametrize("name,kernel,fused", KERNELS)
def test_fold_of_the_pattern_family(gm, world, oracle, name, kernel, fused):
    payloads, meta, fo, hits = world[:4]
    try:
        _setup(gm, world, kernel, fused)
        gm.build_flows()
        res = _check_fold(gm, "patterns", "packet", FM.fold(hits, fo), MM.oracle_counts(oracle, payloads, PATS))
        assert res["timing"].launches == gm.scan_packets()["timing"].launches + 2         # the fold, and the reduce over the folded rows
    finally:
        reset(gm)


def test_fold_of_relations_chains_and_rules(gm, world, oracle):
    payloads, meta, fo, hits, rel, ch, hdr = world
    _setup(gm, world)
    rules = _rules(gm)
    gm.set_rules(rules)
    gm.build_flows()
    counts = MM.oracle_counts(oracle, payloads, PATS)
    mat = np.concatenate([hits, rel, ch, hdr])
    per_packet = MM.rule_rows(mat, rules)
    assert per_packet[1].all() and not per_packet[2].any() and per_packet[3].sum() == 1 and per_packet[4].all() and not per_packet[5].any()
    r = _check_fold(gm, "relations", "packet", FM.fold(rel, fo), counts)
    assert r["timing"].launches == gm.scan_relations()["timing"].launches + 2
    _check_fold(gm, "chains", "packet", FM.fold(ch, fo), counts)
    r = _check_fold(gm, "rules", "packet", FM.fold(per_packet, fo), counts)
    assert r["timing"].launches == gm.scan_rules()["timing"].launches + 2
    # per flow: the terms folded first
    want = FM.flow_rules(mat, fo, rules)
    folded = FM.fold(per_packet, fo)
    assert (want & ~folded).any() and (folded & ~want).any()       # flows a rule matches across payloads only; flows a negated term bars
    assert want[4].all() and not want[5].any() and 0 < want[9].sum() < want.shape[1]
    r = _check_fold(gm, "rules", "flow", want, counts)
    assert r["timing"].launches == gm.scan_rules()["timing"].launches + 2
    # under a profile the fold and what follows it are recorded last: two entries more than the family's own call
    gm.profile_begin(64)
    gm.scan_rules()
    own = len(gm.profile_end(64))
    for scope in ("packet", "flow"):
        gm.profile_begin(64)
        gm.scan_flows("rules", scope)
        assert len(gm.profile_end(64)) == own + 2
    # whole payloads: the rows follow the text rule of the family's own call
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    try:
        sw = MM.starts(payloads, PATS, whole=True)
        _check_fold(gm, "patterns", "packet", FM.fold(MM.hits(sw, len(PATS)), fo))
    finally:
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)


def test_rules_per_flow_by_hand(gm):
    """flow 0: AAA in one payload, BBB in another; 1: AAA alone; 2: BBB alone; 3: AAA, BBB and NEG in three payloads; 4: the chain AAA..BBB in
    one payload, from a source the header predicate names; 5: nothing"""
    texts = {0: [b"AAA", b"-", b"BBB"], 1: [b"AAA"], 2: [b"BBB", b"BBB"], 3: [b"BBB", b"NEG", b"AAA"], 4: [b"AAA BBB"], 5: [b"-", b"-"]}
    order = [0, 3, 1, 0, 2, 3, 5, 4, 0, 2, 3, 5]
    left = {f: list(t) for f, t in texts.items()}
    payloads = [left[f].pop(0) for f in order]
    meta = _meta_of_flows(order, seed=2)
    pats = [b"AAA", b"BBB", b"NEG"]
    chains = [(0, (1, 0, None))]
    heads = [H(src=(A + 4, 0xFFFFFFFF), bidir=True)]
    reset(gm)
    gm.set_patterns(pats)
    load(gm, payloads)
    gm.set_meta(meta)
    gm.set_chains(chains)
    gm.set_headers(heads)
    c0, h0 = gm.chain(0), gm.hdr(0)
    rules = [([0, 1], []), ([0, 1], [2]), ([], [0, 1, 2]), ([c0], []), ([0, h0], []), ([1], [h0, 0])]
    gm.set_rules(rules)
    fo, _ = _check_build(gm, meta, [len(t) for t in payloads], n_flows=6)
    assert fo.tolist() == [0, 1, 2, 0, 3, 1, 4, 5, 0, 3, 1, 4]
    # (the flows are numbered by their first payload: texts' flow 3 is flow 1, 1 is 2, 2 is 3, 5 is 4, 4 is 5)
    st = MM.starts(payloads, pats)
    mat = np.concatenate([MM.hits(st, 3), CM.chain_rows(st, pats, chains), HM.header_rows(meta, [len(t) for t in payloads], heads)])
    want = FM.flow_rules(mat, fo, rules)
    assert want.astype(int).tolist() == [[1, 1, 0, 0, 0, 1],       # AAA and BBB somewhere in the flow
                                         [1, 0, 0, 0, 0, 1],       # ... and NEG nowhere in it
                                         [0, 0, 0, 0, 1, 0],       # none of the three
                                         [0, 0, 0, 0, 0, 1],       # the chain needs one payload
                                         [0, 0, 0, 0, 0, 1],       # a header term
                                         [0, 0, 0, 1, 0, 0]]       # BBB without AAA, not from that source
    _check_fold(gm, "rules", "flow", want)
    # per payload the cross-packet signature fires only where one payload holds both: flow 5's
    per_packet = MM.rule_rows(mat, rules)
    assert np.array_equal(gm.scan_rules(hits=True)["hits"], per_packet) and per_packet[0].sum() == 1
    got = _check_fold(gm, "rules", "packet", FM.fold(per_packet, fo))
    assert got["hits"][0].astype(int).tolist() == [0, 0, 0, 0, 0, 1]
    # SCOPE_FLOW is for rules
    for family in (0, 2, 3):
        assert gm._g.kmpgpu_scan_flows(gm._ctx, family, 1, None, None, None, None, None) == EINVAL


# ------------------------------------------------------------------------------------------------
# 6. kmpgpu_flows_select -> kmpgpu_load_selected
# ------------------------------------------------------------------------------------------------
def test_select_flows_into_load_selected(gm, world):
    payloads, meta, fo = world[:3]
    n, n_flows = len(payloads), int(fo.max()) + 1
    _setup(gm, world)
    gm.build_flows()
    chosen = np.zeros(n_flows, dtype=bool)
    chosen[[0, 7, 8, 31, 39]] = True
    want = FM.expand(chosen, fo)
    assert 0 < want.sum() < n
    words = gm.select_flows(chosen)
    assert words.dtype == np.uint64 and np.array_equal(words, MM.words(want))
    # stray bits at n_flows and above are ignored; a device bitmap gives the same
    stray = MM.words(chosen).copy()
    stray[-1] |= np.uint64(ONES << n_flows & ONES)
    assert np.array_equal(gm.select_flows(stray), words)
    d_bits = torch.from_numpy(stray.view(np.int64)).cuda()
    assert np.array_equal(gm.select_flows(d_bits), words)
    d_words = gm.select_flows(d_bits, device=True)
    assert d_words.is_cuda and np.array_equal(d_words.cpu().numpy().view(np.uint64), words)
    with GpuMatcher(0) as dst:
        for select in (words, d_words):
            idx = dst.load_selected(gm, select)
            assert idx.tolist() == np.flatnonzero(want).tolist()
            a, off, ln = dst.arena_download()
            assert [bytes(a[int(o):int(o) + int(l)]) for o, l in zip(off, ln)] == [payloads[int(k)] for k in idx]
            assert dst.meta().tobytes() == meta[idx.astype(np.int64)].tobytes()
            assert dst.build_flows() == int(chosen.sum())
            sub = meta[idx.astype(np.int64)]
            assert np.array_equal(dst.flow_ids(), FM.flow_of(sub)) and dst.flows().tobytes() == FM.records(sub, ln).tobytes()
    # any[] of scan_flows is what goes in: the whole connections that fired
    gm.set_rules([([0, 1], [])])
    res = gm.scan_flows("rules", "flow")
    assert np.array_equal(gm.select_flows(res["any"]), MM.words(FM.expand(res["any"], fo)))
    # all and none
    assert np.array_equal(gm.select_flows(np.ones(n_flows, dtype=bool)), MM.words(np.ones(n, dtype=bool)))
    assert not gm.select_flows(np.zeros(n_flows, dtype=bool)).any()
    assert gm._g.kmpgpu_flows_select(gm._ctx, None, 0, None, None) == EINVAL
    assert gm._g.kmpgpu_flows_select(gm._ctx, words.ctypes.data, 2, None, None) == EINVAL


# ------------------------------------------------------------------------------------------------
# 7. lifetime and errors
# ------------------------------------------------------------------------------------------------
def _no_flows(m):
    for call in (m.flows, m.flow_ids, lambda: m.scan_flows("patterns"), lambda: m.select_flows(np.zeros(1, dtype=bool))):
        with raises(ESTATE, "no flows"):
            call()


def test_lifetime_and_errors(gm, world):
    payloads, meta, fo, hits = world[:4]
    n, n_flows = len(payloads), int(fo.max()) + 1
    lens = [len(t) for t in payloads]
    reset(gm)
    gm.set_patterns(PATS)
    load(gm, payloads)
    # no metadata; nothing built
    with raises(ESTATE, "no packet metadata"):
        gm.build_flows()
    _no_flows(gm)
    gm.set_meta(meta)
    _no_flows(gm)
    assert gm._g.kmpgpu_flows_build(gm._ctx, 2, None, None) == EINVAL and b"flags" in gm._g.kmpgpu_last_error()
    assert gm._g.kmpgpu_flows_build(None, 0, None, None) == EINVAL
    _check_build(gm, meta, lens)
    # read ranges
    assert gm.flows(n_flows, 0).size == 0 and gm.flow_ids(n, 0).size == 0
    assert gm.flows(3, 2).tobytes() == FM.records(meta, lens)[3:5].tobytes() and np.array_equal(gm.flow_ids(n - 5, 5), fo[n - 5:])
    for first, count in ((0, n_flows + 1), (n_flows, 1), (n_flows + 1, 0), (ONES, 2)):
        with raises(EINVAL, "leave the"):
            gm.flows(first, count)
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0)):
        with raises(EINVAL, "leave the"):
            gm.flow_ids(first, count)
    assert gm._g.kmpgpu_flows_read(gm._ctx, None, 0, 1) == EINVAL
    # unknown family and scope; nothing of the family set
    assert gm._g.kmpgpu_scan_flows(gm._ctx, 4, 0, None, None, None, None, None) == EINVAL
    assert gm._g.kmpgpu_scan_flows(gm._ctx, 0, 2, None, None, None, None, None) == EINVAL
    for family, what in (("rules", "no rules set"), ("relations", "no relations set"), ("chains", "no chains set")):
        with raises(ESTATE, what):
            gm.scan_flows(family)
    # what keeps them: set_patterns, the setters of the row families, options, the on-device repack
    gm.set_patterns(PATS)
    gm.set_relations(RELATIONS)
    gm.set_chains(CHAINS)
    gm.set_headers(HEADS)
    gm.set_rules([([0], [1])])
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    gm.set_option(OPT_WHOLE_PAYLOAD, 0)
    assert np.array_equal(gm.flow_ids(), fo)
    _check_fold(gm, "patterns", "packet", FM.fold(hits, fo))
    # the general kernel cannot mark: the family's own refusal
    gm.set_option(OPT_KERNEL, 1)
    with raises(EINVAL, "streaming kernels only"):
        gm.scan_flows("patterns")
    gm.set_option(OPT_KERNEL, 0)
    # what drops them: set_meta, load_arena, attach_arena
    gm.set_meta(meta)
    _no_flows(gm)
    gm.build_flows()
    gm.set_meta(None)
    _no_flows(gm)
    gm.set_meta(meta)
    gm.build_flows()
    load(gm, payloads)
    _no_flows(gm)
    try:
        # an arena kept in place whose slots are not back to back: the first marking pass packs it, and the flows stay
        gm.set_option(OPT_REPACK, 0)
        slots = [t + b"\xAA" * ((-len(t)) % 16 + 16) for t in payloads]
        keep = attach_slots(gm, payloads, slots)
        _no_flows(gm)
        gm.set_meta(meta)
        _check_build(gm, meta, lens)
        _check_fold(gm, "patterns", "packet", FM.fold(hits, fo))
        assert np.array_equal(gm.flow_ids(), fo) and gm.flows().tobytes() == FM.records(meta, lens).tobytes()
        del keep
    finally:
        gm.set_option(OPT_REPACK, 1)
    # between kmpgpu_load_frames_begin and _finish
    fr = _lib.Frames()
    err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
    assert _lib.host_lib().kmp_frames_from_pcap(os.path.join(DATA, "udp_1000.pcap").encode(), None, None, C.byref(fr), err) == 0
    try:
        with GpuMatcher(0) as other:
            other.set_patterns(PATS)
            assert other._g.kmpgpu_load_frames_begin(other._ctx, fr.bytes, fr.nbytes, fr.off, fr.caplen, fr.n, 0) == 0
            with raises(ESTATE, "kmpgpu_load_frames_begin"):
                other.build_flows()
            n_pay = C.c_uint64()
            assert other._g.kmpgpu_load_frames_finish(other._ctx, C.byref(n_pay)) == 0
    finally:
        _lib.host_lib().kmp_frames_free(C.byref(fr))


def test_no_payloads(gm):
    reset(gm)
    gm.set_patterns(PATS)
    gm.load_arena(HostArena.from_payloads([]))
    assert gm.build_flows() == 0 and gm.flows().size == 0 and gm.flow_ids().size == 0
    res = gm.scan_flows("patterns", hits=True)
    assert res["flow_counts"].tolist() == [0] * len(PATS) and res["hits"].shape == (len(PATS), 0) and res["timing"].launches == 0
    assert gm.select_flows(np.zeros(0, dtype=bool)).size == 0
    with raises(EINVAL, "leave the"):
        gm.flows(0, 1)


# ------------------------------------------------------------------------------------------------
# 8. every other call is what it was
# ------------------------------------------------------------------------------------------------
def test_other_calls_are_untouched(gm, world):
    _setup(gm, world)
    gm.set_rules(_rules(gm))

    def snapshot():
        out = []
        c, t = gm.scan()
        out.append((c.tobytes(), t.launches, gm.last_timing().launches))
        for res in (gm.scan_packets(hits=True), gm.scan_rules(hits=True)):
            out.append((res["hits"].tobytes(), res["any"].tobytes(), res["counts"].tobytes(), res["timing"].launches))
        al = gm.scan_alerts("rules")
        out.append((al["alerts"].tobytes(), al["n_found"], al["n_packets"], al["pkt_counts"].tobytes(), al["timing"].launches))
        return out

    before = snapshot()
    n_flows = gm.build_flows()
    gm.scan_flows("patterns", hits=True)
    gm.scan_flows("rules", "flow", hits=True)
    gm.select_flows(np.ones(n_flows, dtype=bool))
    assert snapshot() == before


# ------------------------------------------------------------------------------------------------
# 9. the command lines: KMPGPU_FLOWS_FILE, KMPGPU_FLOW_ALERTS_FILE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"])])
def test_cli_flow_files(tokens, tmp_path, prog, extra, directed):
    pay, meta = HM.capture(HM.pcap_frames(os.path.join(DATA, "big_udp.pcap")), "udp")
    lens = [len(t) for t in pay]
    hits = MM.hits(MM.starts(pay, tokens), len(tokens))
    rules = [([3, 53], []), ([3], [1]), ([], [2, 3])]      # two tokens that meet in one flow without meeting in a payload; a negation; only negations
    fo = FM.flow_of(meta, directed)
    want = FM.flow_rules(hits, fo, rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size
    assert (want[0] & ~FM.fold(MM.rule_rows(hits, rules), fo)[0]).any()          # flows the first rule matches across payloads only
    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([str(i) for i in pos] + ["!" + str(i) for i in neg]) + "\n" for pos, neg in rules))
    plain = run_cli(prog, "big_udp.pcap", extra=extra)
    assert plain.returncode == 0, plain.stderr
    files = []
    for route in ("0", "1"):
        ff, fa = tmp_path / f"flows{route}.csv", tmp_path / f"flow_alerts{route}.csv"
        r = run_cli(prog, "big_udp.pcap", extra=extra, env_extra={"KMPGPU_FLOWS_FILE": str(ff), "KMPGPU_FLOW_ALERTS_FILE": str(fa), "KMPGPU_RULES_FILE": str(rf),
                                                                  "KMPGPU_FLOWS_DIRECTED": "1" if directed else "0", "KMPGPU_DEVICE_EXTRACT": route})
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == strip_elapsed(plain.stdout)
        files.append((ff.read_text(), fa.read_text()))
    assert files[0][0] == FM.flows_file(FM.records(meta, lens, directed))
    assert files[0][1] == FM.flow_alerts_file(want)
    assert files[0] == files[1]                            # host extraction and device extraction write the same bytes
