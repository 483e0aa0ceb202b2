"""Flow streams by TCP sequence number on the GPU (kmpgpu_load_streams_ordered, kmpgpu_stream_segs_read, kmpgpu_stream_orders_read;
include/kmpgpu.h) against tests/stream_seq_model.py, an independent model written from the definition (a dict of cells per stream, no
running maximum).  Every comparison is exact: the arena byte for byte, index, metadata and all four record arrays.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gpu_support import (FLOW_A as A, FLOW_B as B, attach_slots, gm, load, meta_of_flows, reset, torch)  # noqa: F401  (gm: the context fixture)

import header_model as HM
import stream_model as TM
import stream_seq_model as QM
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import HostArena
from multithreading_string_matching_amd.matcher import (OPT_NONTEMPORAL, OPT_REPACK, OPT_WHOLE_PAYLOAD, STREAM_DEPTH_MAX, STREAM_ORDER_DTYPE,
                                                        STREAM_SEG_DTYPE, GpuMatcher, stream_locate_ordered)

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
FULL = 1 << 30
X, Y, Z = (A, 40000, B, 80), (B, 80, A, 40000), (A + 1, 40001, B, 80)


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


def _meta(rows, proto=6):
    m = np.zeros(len(rows), dtype=HM.META_DTYPE)
    for k, (s, sp, d, dp) in enumerate(rows):
        m[k]["src_ip"], m[k]["src_port"], m[k]["dst_ip"], m[k]["dst_port"], m[k]["proto"] = s, sp, d, dp, proto
    return m


@pytest.fixture(scope="module")
def sm():
    """the second context: the one that owns the streams"""
    m = GpuMatcher(0)
    yield m
    m.close()


def cut(model, depth):
    """the model built at the full depth, cut to `depth`: only the streams' bytes and len depend on it"""
    streams, recs, pos, segs, orders, origin = model
    recs = recs.copy()
    recs["len"] = np.minimum(recs["bytes"], depth)
    return [s[:depth] for s in streams], recs, pos, segs, orders


def check(dst, model, meta, depth):
    """dst's arena, index, metadata and the four record arrays against the model's, byte for byte"""
    streams, recs, pos, segs, orders = cut(model, depth)
    want, off, ln = TM.arena(streams)
    got, gmap, gsegs, gorders = dst.streams(), dst.stream_map(), dst.stream_segs(), dst.stream_orders()

    def differ(a, b):
        """the first records that differ, as (index, got, wanted)"""
        return [(i, x, y) for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())) if x != y][:3]

    assert got.tobytes() == recs.tobytes(), differ(got, recs)
    assert gmap.tobytes() == pos.tobytes(), differ(gmap, pos)
    assert gsegs.dtype == STREAM_SEG_DTYPE and gsegs.tobytes() == segs.tobytes(), differ(gsegs, segs)
    assert gorders.dtype == STREAM_ORDER_DTYPE and gorders.tobytes() == orders.tobytes(), differ(gorders, orders)
    assert dst.arena_info() == (len(streams), sum(len(s) for s in streams))
    a, o, l = dst.arena_download()
    assert np.array_equal(o, off) and np.array_equal(l, ln) and ln.tolist() == recs["len"].tolist()
    assert len(a) >= len(want) and not a[len(want):].any()
    bad = np.flatnonzero(a[:len(want)] != want)
    assert bad.size == 0, [(int(b), int(np.searchsorted(off, b, side="right")) - 1, int(a[b]), int(want[b])) for b in bad[:8]]
    assert dst.meta().tobytes() == meta[recs["first_packet"].astype(np.int64)].tobytes()
    return streams, recs


def _put(src, pay, meta, form):
    """the source loaded; attached with dirty slot padding; attached with gaps between the slots and kept in place"""
    keep = None
    if form == "loaded":
        load(src, pay)
    elif form == "dirty":
        keep = attach_slots(src, pay, [t + b"\xAA" * (TM.slot(len(t)) - len(t)) for t in pay])
    else:
        src.set_option(OPT_REPACK, 0)
        keep = attach_slots(src, pay, [t + b"\xBB" * (TM.slot(len(t)) - len(t) + 16 * (k % 3)) for k, t in enumerate(pay)])
    src.set_meta(meta)
    return keep


def _flows(seed, n=3000, n_flows=40):
    """about 3 000 payloads in 40 flows, both directions, every third flow UDP"""
    rng = np.random.default_rng(seed)
    flow = np.concatenate([np.arange(n_flows), rng.integers(0, n_flows, n - n_flows)])
    meta = meta_of_flows(flow, seed=seed)
    meta["proto"] = np.where(flow % 3 == 0, 17, 6)
    return rng, meta


def _isn(rng, s):
    return (1 << 32) - int(rng.integers(1, 500)) if s % 3 == 0 else int(rng.integers(0, 1 << 32))


# ------------------------------------------------------------------------------------------------
# 1. sequence numbers that agree with capture order: everything kmpgpu_load_streams gives
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _in_order():
    rng, meta = _flows(21)
    lens = rng.integers(0, 201, len(meta))
    pay = [bytes(rng.integers(1, 256, int(x), dtype=np.uint8)) for x in lens]
    seq = np.zeros(len(meta), dtype=np.uint32)
    for s, (f, d, ks) in enumerate(TM.members(meta)):
        at = _isn(rng, s)
        for k in ks:
            seq[k] = at & 0xFFFFFFFF
            at += len(pay[k])
    return pay, meta, seq


@pytest.mark.parametrize("depth", [1, 17, 4096, FULL])
def test_in_order_equals_load_streams(gm, sm, depth):
    pay, meta, seq = _in_order()
    reset(gm, sm)
    gm.set_patterns([b"x"])
    load(gm, pay)
    gm.set_meta(meta)
    gm.build_flows()

    def snapshot():
        a, off, ln = sm.arena_download()
        return a.tobytes(), off.tobytes(), ln.tobytes(), sm.meta().tobytes(), sm.streams().tobytes(), sm.stream_map().tobytes()

    n = sm.load_streams(gm, depth)
    plain = snapshot()
    with raises(ESTATE, "kmpgpu_stream_segs_read: no sequence order"):
        sm.stream_segs()
    with raises(ESTATE, "kmpgpu_stream_orders_read: no sequence order"):
        sm.stream_orders()
    assert sm.load_streams(gm, depth, seq=seq) == n
    assert snapshot() == plain
    t = sm.last_timing()
    assert t.launches == 16 and t.kernel_ms > 0
    segs, orders = sm.stream_segs(), sm.stream_orders()
    assert not segs["skip"].any() and segs["take"].tolist() == [len(t) for t in pay]
    assert not orders["n_gaps"].any() and not orders["gap_bytes"].any() and not orders["dup_bytes"].any()
    recs = sm.streams()
    assert orders["tcp"].tolist() == (meta["proto"][recs["first_packet"].astype(np.int64)] == 6).astype(int).tolist()
    assert 0 < orders["tcp"].sum() < n
    # the same from a device tensor
    d_seq = torch.from_numpy(seq.view(np.int32)).cuda()
    assert sm.load_streams(gm, depth, seq=d_seq) == n
    assert snapshot() == plain and sm.stream_segs().tobytes() == segs.tobytes() and sm.stream_orders().tobytes() == orders.tobytes()


# ------------------------------------------------------------------------------------------------
# 2. members permuted, duplicated, overlapping, empty: against the model
# ------------------------------------------------------------------------------------------------
def _segments(rng, m, lengths, gap=0.03):
    """m segments (offset in the stream's sequence space, bytes): 20 % exact duplicates of an earlier one, 10 % partial overlaps that start
    1..40 bytes in front of what was sent so far (with bytes of their own: which copy is kept shows), some empty ones, a few holes"""
    segs, at = [], 0
    for _ in range(m):
        r = rng.random()
        if segs and r < 0.2:
            segs.append(segs[int(rng.integers(len(segs)))])
        elif at > 0 and r < 0.3:
            back = min(at, int(rng.integers(1, 41)))
            body = bytes(rng.integers(1, 256, int(rng.choice(lengths)), dtype=np.uint8))
            segs.append((at - back, body))
            at = max(at, at - back + len(body))
        elif r < 0.35:
            segs.append((at, b""))
        else:
            if r > 1 - gap:
                at += int(rng.integers(1, 30))
            body = bytes(rng.integers(1, 256, int(rng.choice(lengths)), dtype=np.uint8))
            segs.append((at, body))
            at += len(body)
    return segs


def _spread(rng, meta, lengths):
    """every stream's segments handed to its members in a random order"""
    pay, seq = [b""] * len(meta), np.zeros(len(meta), dtype=np.uint32)
    for s, (f, d, ks) in enumerate(TM.members(meta)):
        isn = _isn(rng, s)
        segs = _segments(rng, len(ks), lengths)
        for k, j in zip(ks, rng.permutation(len(ks))):
            pay[k], seq[k] = segs[j][1], (isn + segs[j][0]) & 0xFFFFFFFF
    return pay, seq


@functools.lru_cache(maxsize=None)
def _disordered():
    rng, meta = _flows(22)
    pay, seq = _spread(rng, meta, np.arange(0, 201))
    model = QM.build(pay, meta, seq, FULL)
    orders, segs = model[4], model[3]
    assert orders["n_gaps"].sum() > 20 and orders["dup_bytes"].sum() > 10000 and (segs["take"] == 0).sum() > 300
    assert ((segs["skip"] > 0) & (segs["take"] > 0)).sum() > 100
    return pay, meta, seq, model


@pytest.mark.parametrize("form", ["loaded", "dirty", "in_place"])
@pytest.mark.parametrize("depth", [1, 15, 16, 17, 100, FULL])
def test_against_the_model(gm, sm, depth, form):
    pay, meta, seq, model = _disordered()
    reset(gm, sm)
    try:
        gm.set_patterns([b"x"])
        keep = _put(gm, pay, meta, form)
        n_flows = gm.build_flows()
        n = sm.load_streams(gm, depth, seq=seq)
        streams, recs = check(sm, model, meta, depth)
        assert n == len(recs)
        # the flow identity
        assert sm.build_flows() == n_flows and sm.flow_ids().tolist() == recs["flow"].tolist()
        # read ranges
        for read, m in ((sm.stream_segs, len(pay)), (sm.stream_orders, n)):
            assert read(m, 0).size == 0 and read(3, 2).tobytes() == read()[3:5].tobytes()
            for first, count in ((0, m + 1), (m, 1), (m + 1, 0)):
                with raises(EINVAL, "leave the"):
                    read(first, count)
        del keep
    finally:
        reset(gm, sm)


def test_default_cache_policy(gm, sm):
    """OPT_NONTEMPORAL = 0 on the context that receives the streams: the other instantiation of the gather kernel"""
    pay, meta, seq, model = _disordered()
    reset(gm, sm)
    try:
        sm.set_option(OPT_NONTEMPORAL, 0)
        gm.set_patterns([b"x"])
        keep = _put(gm, pay, meta, "dirty")
        gm.build_flows()
        for depth in (17, 4096):
            sm.load_streams(gm, depth, seq=seq)
            check(sm, model, meta, depth)
        del keep
    finally:
        reset(gm, sm)


# ------------------------------------------------------------------------------------------------
# 3. the scans' tiles (KMP_SCAN_TILE = 1024)
# ------------------------------------------------------------------------------------------------
def _retransmitting(rng, m):
    """m members in order, every third the member before it once more"""
    out, at = [], 0
    for i in range(m):
        if i % 3 == 2:
            out.append(out[-1])
        else:
            body = bytes(rng.integers(1, 256, int(rng.integers(1, 20)), dtype=np.uint8))
            out.append((at, body))
            at += len(body)
    return out


@pytest.mark.parametrize("sizes", [(2500,), (1024, 5, 7, 9, 1500)], ids=["one_stream", "head_at_1024"])
def test_scan_tiles(gm, sm, sizes):
    """The running maximum and the sums carry across tiles; a stream head exactly at sorted position 1024; three streams inside one tile."""
    rng = np.random.default_rng(len(sizes))
    rows, pay, seq = [], [], []
    for f, m in enumerate(sizes):                               # flows are numbered by their first payload: sorted order is this order
        for off, body in _retransmitting(rng, m):
            rows.append((A + f, 1000, B, 80))
            pay.append(body)
            seq.append((0xFFFFFF00 + off) & 0xFFFFFFFF)
    meta, seq = _meta(rows), np.array(seq, dtype=np.uint32)
    model = QM.build(pay, meta, seq, FULL)
    assert model[4]["dup_bytes"].all() and model[1]["n_packets"].tolist() == list(sizes)
    reset(gm, sm)
    gm.set_patterns([b"x"])
    load(gm, pay)
    gm.set_meta(meta)
    gm.build_flows()
    for depth in (FULL, 4097):
        assert sm.load_streams(gm, depth, seq=seq) == len(sizes)
        check(sm, model, meta, depth)


# ------------------------------------------------------------------------------------------------
# 4. many pieces per unit: 1-byte members with covered duplicates between them
# ------------------------------------------------------------------------------------------------
def test_many_pieces_in_one_unit(gm, sm):
    rng = np.random.default_rng(4)
    rows, pay, seq = [], [], []
    for i in range(300):
        body = bytes(rng.integers(1, 256, 1, dtype=np.uint8))
        for _ in range(1 + int(rng.integers(0, 4))):            # the byte, then 0..3 covered copies of it
            rows.append(X)
            pay.append(body)
            seq.append(5 + i)
    for i in range(40):                                         # a second stream: 3-byte members, each overlapping the one before by 2
        rows.append(Z)
        pay.append(bytes(rng.integers(1, 256, 3, dtype=np.uint8)))
        seq.append(900 + i)
    order = rng.permutation(len(rows))
    rows, pay, seq = [rows[i] for i in order], [pay[i] for i in order], np.array(seq, dtype=np.uint32)[order]
    meta = _meta(rows)
    model = QM.build(pay, meta, seq, FULL)
    assert [len(s) for s in model[0]] == [300, 42] or [len(s) for s in model[0]] == [42, 300]
    reset(gm, sm)
    gm.set_patterns([b"x"])
    for form in ("loaded", "dirty"):
        keep = _put(gm, pay, meta, form)
        gm.build_flows()
        for depth in (FULL, 50, 33):
            assert sm.load_streams(gm, depth, seq=seq) == 2
            check(sm, model, meta, depth)
        del keep


# ------------------------------------------------------------------------------------------------
# 5. a borrowed arena that ends with its last slot, whose last member is half covered
# ------------------------------------------------------------------------------------------------
def test_last_slot_of_a_borrowed_arena(gm, sm):
    pay = [b"a" * 31, b"b" * 5, b"c" * 32]
    seq = (0xFFFFFFF0 + np.array([0, 47, 15], dtype=np.uint64)).astype(np.uint32)             # the last one: 16 bytes covered, 16 kept
    meta = _meta([X, X, X])
    ln = np.array([len(t) for t in pay], dtype=np.uint32)
    off = np.array([0, 32, 48], dtype=np.uint64)
    arena = np.frombuffer(pay[0] + b"\xCC" + pay[1] + b"\xCC" * 11 + pay[2], dtype=np.uint8).copy()
    assert len(arena) == 80
    keep = (torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    model = QM.build(pay, meta, seq, FULL)
    assert model[0] == [b"a" * 31 + b"c" * 16 + b"b" * 5] and model[3]["skip"].tolist() == [0, 0, 16]
    reset(gm, sm)
    gm.set_patterns([b"x"])
    gm.attach_arena(*keep)
    gm.set_meta(meta)
    gm.build_flows()
    for depth in (3, 31, 32, 46, 47, 48, 52, 100):
        assert sm.load_streams(gm, depth, seq=seq) == 1
        check(sm, model, meta, depth)
    del keep


# ------------------------------------------------------------------------------------------------
# 6. what the order is for
# ------------------------------------------------------------------------------------------------
def test_semantics_end_to_end(gm, sm):
    # flow 0: "GET /admin HTTP" in three segments captured out of order, the server's answers in between
    # flow 1: a content sent twice (a retransmission), then a second content whose offset the duplicate moves
    pay = [b"in HTTP", b"200", b"GET /", b"OK", b"adm", b"....EVIL", b"EVIL", b"..TAIL"]
    rows = [X, Y, X, Y, X, Z, Z, Z]
    seq = np.array([1008, 50, 1000, 53, 1005, 7000, 7004, 7008], dtype=np.uint32)
    pats = [b"/admin", b"EVIL", b"TAIL"]
    rules = [([0], []), ([1], []), ([2], [])]
    reset(gm, sm)
    try:
        for m in (gm, sm):
            m.set_option(OPT_WHOLE_PAYLOAD, 1)
            m.set_patterns(pats)
        load(gm, pay)
        gm.set_meta(_meta(rows))
        assert gm.build_flows() == 2
        sm.set_rules(rules)
        sm.set_windows([(0, None), (0, None), (10, 10)])         # TAIL at offset 10 of the de-duplicated stream, 14 with the copy in it
        # capture order: /admin is not contiguous, EVIL counts twice, TAIL is at 14
        sm.load_streams(gm)
        assert sm.build_flows() == 2
        res = sm.scan_flows("rules", "flow", hits=True)
        assert res["hits"].tolist() == [[False, False], [False, True], [False, False]] and res["counts"].tolist() == [0, 2, 1]
        # sequence order
        sm.load_streams(gm, seq=seq)
        assert sm.build_flows() == 2
        a, off, ln = sm.arena_download()
        assert [bytes(a[int(o):int(o) + int(l)]) for o, l in zip(off, ln)] == [b"GET /admin HTTP", b"200OK", b"....EVIL..TAIL"]
        res = sm.scan_flows("rules", "flow", hits=True)
        assert res["hits"].tolist() == [[True, False], [False, True], [False, True]] and res["counts"].tolist() == [1, 1, 1]
        assert sm.stream_orders()["dup_bytes"].tolist() == [0, 0, 4]
    finally:
        sm.set_windows(None)
        reset(gm, sm)


# ------------------------------------------------------------------------------------------------
# 7. offsets map back
# ------------------------------------------------------------------------------------------------
def test_offsets_map_back(gm, sm):
    rng = np.random.default_rng(8)
    n, n_flows = 400, 12
    pats = [b"ab", b"abc", b"cab", b"a"]
    flow = np.concatenate([np.arange(n_flows), rng.integers(0, n_flows, n - n_flows)])
    meta = meta_of_flows(flow, seed=8)
    meta["proto"] = np.where(flow % 4 == 0, 17, 6)
    # one underlying text per stream, so that overlapping copies agree and a match may lie across any number of members
    pay, seq = [b""] * n, np.zeros(n, dtype=np.uint32)
    for s, (f, d, ks) in enumerate(TM.members(meta)):
        text = bytes(rng.choice([0x61, 0x62, 0x63], 40 * len(ks), p=[.4, .4, .2]).astype(np.uint8))
        at, isn = 0, _isn(rng, s)
        for k in rng.permutation(ks):
            lo = max(0, at - int(rng.integers(0, 6)))
            hi = lo + int(rng.integers(0, 12))
            pay[k], seq[k], at = text[lo:hi], (isn + lo) & 0xFFFFFFFF, max(at, hi)
    reset(gm, sm)
    try:
        for m in (gm, sm):
            m.set_option(OPT_WHOLE_PAYLOAD, 1)
            m.set_patterns(pats)
        load(gm, pay)
        gm.set_meta(meta)
        gm.build_flows()
        sm.load_streams(gm, FULL, seq=seq)
        got = sm.scan_offsets(200000)[0]
        assert len(got) > 1000
        smap, segs = sm.stream_map(), sm.stream_segs()
        members = 0
        for j in range(4):                                      # byte j of every match whose pattern has one
            has = np.array([len(pats[int(i)]) > j for i in got["pattern"]])
            k, o = stream_locate_ordered(smap, segs, got["packet"][has], got["offset"][has].astype(np.int64) + j)
            want = [pats[int(i)][j] for i in got["pattern"][has]]
            assert [pay[int(a)][int(b)] for a, b in zip(k, o)] == want
            if j == 0:
                first = dict(zip(np.flatnonzero(has).tolist(), k.tolist()))
            else:
                members += sum(first[i] != kk for i, kk in zip(np.flatnonzero(has).tolist(), k.tolist()))
        assert members > 50                                     # matches that start in one member and go on in another
    finally:
        reset(gm, sm)


# ------------------------------------------------------------------------------------------------
# 8. two builds, src untouched, errors, state
# ------------------------------------------------------------------------------------------------
def test_two_builds_are_byte_identical_and_src_is_untouched(gm, sm):
    pay, meta, seq, model = _disordered()
    reset(gm, sm)
    gm.set_patterns([b"\x41", bytes([7, 9])])
    load(gm, pay)
    gm.set_meta(meta)
    gm.set_rules([([0], [1])])
    gm.build_flows()

    def snapshot():
        res = gm.scan_flows("rules", "flow", hits=True)
        a, off, ln = gm.arena_download()
        return (res["hits"].tobytes(), res["counts"].tobytes(), a.tobytes(), off.tobytes(), ln.tobytes(), gm.meta().tobytes(),
                gm.flow_ids().tobytes(), gm.flows().tobytes())

    before = snapshot()
    outs = []
    for _ in range(2):
        sm.load_streams(gm, 300, seq=seq)
        a, off, ln = sm.arena_download()
        outs.append((a.tobytes(), off.tobytes(), ln.tobytes(), sm.meta().tobytes(), sm.streams().tobytes(), sm.stream_map().tobytes(),
                     sm.stream_segs().tobytes(), sm.stream_orders().tobytes()))
    assert outs[0] == outs[1]
    assert snapshot() == before
    gm.set_rules([])


def test_errors_and_state(gm, sm):
    pay, meta, seq = _in_order()
    pay, meta, seq = pay[:200], meta[:200], seq[:200]
    G = gm._g
    reset(gm, sm)
    for m in (gm, sm):
        m.set_patterns([b"ab"])
    load(gm, pay)
    load(sm, [b"kept"])
    n = C.c_uint64(99)
    ptr = seq.ctypes.data

    def kept():
        a, off, ln = sm.arena_download()
        return sm.arena_info() == (1, 4) and bytes(a[:4]) == b"kept"

    with raises(ESTATE, "kmpgpu_load_streams_ordered: src has no metadata"):
        sm.load_streams(gm, seq=seq)
    gm.set_meta(meta)
    with raises(ESTATE, "kmpgpu_load_streams_ordered: no flows"):
        sm.load_streams(gm, seq=seq)
    gm.build_flows()
    assert G.kmpgpu_load_streams_ordered(sm._ctx, sm._ctx, 16, ptr, 0, C.byref(n)) == EINVAL and b"dst and src are the same" in G.kmpgpu_last_error()
    assert n.value == 0
    assert G.kmpgpu_load_streams_ordered(None, gm._ctx, 16, ptr, 0, None) == EINVAL and G.kmpgpu_load_streams_ordered(sm._ctx, None, 16, ptr, 0, None) == EINVAL
    assert b"kmpgpu_load_streams_ordered: ctx is NULL" in G.kmpgpu_last_error()
    for depth in (0, STREAM_DEPTH_MAX + 1, 0xFFFFFFFF):
        with raises(EINVAL, "kmpgpu_load_streams_ordered: depth"):
            sm.load_streams(gm, depth, seq=seq)
    assert G.kmpgpu_load_streams_ordered(sm._ctx, gm._ctx, 16, None, 0, None) == EINVAL and b"seq is NULL" in G.kmpgpu_last_error()
    for on_device in (2, -1):
        assert G.kmpgpu_load_streams_ordered(sm._ctx, gm._ctx, 16, ptr, on_device, None) == EINVAL and b"on_device" in G.kmpgpu_last_error()
    assert kept()
    for read in (sm.stream_segs, sm.stream_orders):
        with raises(ESTATE, "no streams"):
            read()
    assert G.kmpgpu_stream_segs_read(None, None, 0, 0) == EINVAL and G.kmpgpu_stream_orders_read(None, None, 0, 0) == EINVAL
    with pytest.raises(ValueError, match="sequence numbers for"):
        sm.load_streams(gm, seq=seq[:-1])
    # built; whatever replaces dst's arena drops the state, a plain build drops the order
    assert sm.load_streams(gm, 64, seq=seq) > 40
    assert sm.stream_segs().size == 200
    assert G.kmpgpu_stream_segs_read(sm._ctx, None, 0, 1) == EINVAL and G.kmpgpu_stream_orders_read(sm._ctx, None, 0, 1) == EINVAL
    load(sm, [b"kept"])
    with raises(ESTATE, "kmpgpu_stream_segs_read: no streams"):
        sm.stream_segs()
    sm.load_streams(gm, 64, seq=seq)
    sm.load_streams(gm, 64)
    with raises(ESTATE, "kmpgpu_stream_orders_read: no sequence order"):
        sm.stream_orders()
    # n_pkts == 0
    gm.load_arena(HostArena.from_payloads([]))
    assert gm.build_flows() == 0
    load(sm, [b"kept"])
    assert G.kmpgpu_load_streams_ordered(sm._ctx, gm._ctx, 64, None, 0, C.byref(n)) == 0 and n.value == 0
    assert sm.arena_info() == (0, 0)
    load(sm, [b"kept"])
    assert sm.load_streams(gm, 64, seq=np.zeros(0, dtype=np.uint32)) == 0
    assert sm.arena_info() == (0, 0) and sm.stream_segs().size == 0 and sm.stream_orders().size == 0 and sm.last_timing().launches == 0
