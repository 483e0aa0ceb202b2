"""Header predicates on the GPU (kmpgpu_set_headers / kmpgpu_scan_headers, include/kmpgpu.h) and the per-payload metadata they read
(KMPGPU_OPT_KEEP_META, kmpgpu_set_meta, kmpgpu_load_selected), against tests/header_model.py: an independent numpy model written from
the byte rules and the predicate's definition.

The value domains are small -- 4 addresses, 6 ports, protocols {6, 17, 1}, lengths {0, 1, 40, 1500} -- so that no row of the model is
trivially empty or full; every test asserts that on the model's rows before it looks at the device's.
"""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN

from gpu_support import KERNELS, attach_slots, gm, load, reset, run_cli, strip_elapsed, torch  # noqa: F401  (gm: the context fixture)

import chain_model as CM
import header_model as HM
import match_model as MM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import META_DTYPE, HostArena
from multithreading_string_matching_amd.matcher import OPT_FUSED, OPT_KEEP_META, OPT_KERNEL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
TILE = 256 * 4                # KMP_SCAN_TILE
HDR_TILE = _lib.HDR_TILE      # predicates the header kernel stages at a time
U32 = 0xFFFFFFFF

ADDR = [0x0A000001, 0x0A800002, 0xC0A80101, 0xAC100A0A]      # 10.0.0.1, 10.128.0.2, 192.168.1.1, 172.16.10.10
PORTS = [0, 53, 80, 1024, 40000, 65535]
PROTOS = [6, 17, 1]
LENS = [0, 1, 40, 1500]
PATS = [b"GET", b"/admin", b"xyz"]
N_MAX = 4097
H = HM.header


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


# ------------------------------------------------------------------------------------------------
# one synthetic capture, shared: payload k has a length of LENS and header fields of the domains; payloads 0 .. 3 are planted
# ------------------------------------------------------------------------------------------------
def _text(rng, length):
    body = [b"GET /admin HTTP/1.1 xyz ", b"POST /admin xyz GET ", b"xyz xyz nothing here ", b"get /ADMIN \0 GET /admin xyz "][int(rng.integers(4))]
    return (body * (length // len(body) + 1))[:length]


def _capture(n, seed=7):
    rng = np.random.default_rng(seed)
    meta = np.zeros(n, dtype=META_DTYPE)
    meta["src_ip"] = rng.choice(ADDR, n)
    meta["dst_ip"] = rng.choice(ADDR, n)
    meta["src_port"] = rng.choice(PORTS, n)
    meta["dst_port"] = rng.choice(PORTS, n)
    meta["proto"] = rng.choice(PROTOS, n)
    lens = rng.choice(LENS, n)
    # payload 0: udp, so that the first predicate (udp) holds for it and the second (tcp) does not; 2 and 3: one flow, forwards and back
    plant = [(ADDR[1], ADDR[3], 80, 1024, 17, 40), (ADDR[0], ADDR[1], 0, 0, 6, 0), (ADDR[2], ADDR[0], 40000, 53, 17, 1500), (ADDR[0], ADDR[2], 53, 40000, 17, 1500)]
    for k, (s, d, sp, dp, pr, ln) in enumerate(plant[:n]):
        meta[k] = (s, d, sp, dp, pr, (0, 0, 0))
        lens[k] = ln
    payloads = [_text(rng, int(l)) for l in lens]
    return payloads, meta


def _predicates(n):
    """n predicates: the cases the kernel can get wrong first, then draws from the domains"""
    fixed = [
        H(proto=17),                                                            # exact protocol
        H(proto=6),
        H(),                                                                    # any / any
        H(src=(0xDEADBEEF, 0), dport=(53, 53)),                                 # /0: the address is not looked at
        H(src=(ADDR[0], U32)),                                                  # /32
        H(src=(0x0A000000, 0xFF800000)),                                        # /9: 10.0.0.1, not 10.128.0.2
        H(dst=(0x0A000002, 0xFF0000FF)),                                        # a non-contiguous mask: 10.x.y.2
        H(sport=(53, 53)),                                                      # lo == hi
        H(proto=1, sport=(0, 65535), dport=(0, 65535)),                         # 0:65535
        H(dport=(0, 0)),                                                        # port 0
        H(proto=17, src=(ADDR[2], U32), sport=(40000, 40000), dst=(ADDR[0], U32), dport=(53, 53), bidir=True),    # the flow of payloads 2 and 3
        H(proto=17, src=(ADDR[2], U32), sport=(40000, 40000), dst=(ADDR[0], U32), dport=(53, 53)),                # ... one way only
        H(length=(0, 0)),                                                       # empty payloads
        H(length=(1500, U32)),                                                  # lo:UINT32_MAX
        H(proto=6, length=(1, 40)),
        H(sport=(1024, 65535), dport=(0, 1023), bidir=True),
    ]
    rng = np.random.default_rng(11)
    out = list(fixed)
    while len(out) < n:
        out.append(H(proto=[None, 6, 17, 1][int(rng.integers(4))], src=(int(rng.choice(ADDR)), [0, U32, 0xFF000000, 0xFFFF0000][int(rng.integers(4))]),
                     dst=(int(rng.choice(ADDR)), [0, 0, U32, 0xFF000000][int(rng.integers(4))]),
                     sport=tuple(sorted(int(x) for x in rng.choice(PORTS, 2))), dport=[(0, 65535), (53, 80), (1024, 65535)][int(rng.integers(3))],
                     length=[(0, U32), (0, 1), (40, 1500), (1, U32)][int(rng.integers(4))], bidir=bool(rng.integers(2))))
    return out[:n]


@pytest.fixture(scope="module")
def world():
    """payloads, metadata, predicates and the model's rows for the largest case; every test slices it"""
    payloads, meta = _capture(N_MAX)
    heads = _predicates(HDR_TILE + 1)
    lens = np.array([len(t) for t in payloads])
    rows = HM.header_rows(meta, lens, heads)
    assert 0 < rows.sum() < rows.size
    for q in range(len(heads)):
        assert rows[q].any(), (q, heads[q])
        assert q == 2 or not rows[q].all(), (q, heads[q])
    # the flow: payload 3 is payload 2's answer, and only the swap makes the predicate hold for it
    assert rows[10, 2] and rows[10, 3] and rows[11, 2] and not rows[11, 3]
    # empty payloads are there and hit
    assert (lens == 0).any() and rows[12].sum() == (lens == 0).sum()
    return payloads, meta, heads, rows


def _not_trivial(rows):
    if rows.size == 1:
        assert rows.sum() == 1
    else:
        assert 0 < rows.sum() < rows.size


def _check_headers(m, rows, counts=None):
    res = m.scan_headers(hits=True)
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, [(int(q), int(k), bool(rows[q, k])) for q, k in bad[:8]]
    assert res["hdr_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    if counts is not None:
        assert res["counts"].tolist() == list(counts)
    return res


# ------------------------------------------------------------------------------------------------
# 1. predicate rows against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hdr", [1, 2, 63, 64, 65, HDR_TILE + 1])
@pytest.mark.parametrize("n_pkts", [1, 63, 64, 65, 127, 128, 129, N_MAX])
def test_rows_against_the_model(gm, world, n_pkts, n_hdr):
    payloads, meta, heads, rows = world
    rows = rows[:n_hdr, :n_pkts]
    _not_trivial(rows)
    reset(gm)
    gm.set_patterns(PATS)
    load(gm, payloads[:n_pkts])
    gm.set_meta(meta[:n_pkts])
    gm.set_headers(heads[:n_hdr])
    res = _check_headers(gm, rows)
    # the marking pass and the header kernel
    plain = gm.scan_packets()
    assert res["timing"].launches == plain["timing"].launches                   # (the header kernel in the reduce's place)
    assert res["counts"].tolist() == plain["counts"].tolist()
    # the raw words: the bits at n_pkts and above are 0
    W = (n_pkts + 63) // 64
    hit_w = np.full((n_hdr, W), U32 << 32 | U32, dtype=np.uint64)
    any_w = np.full(W, U32 << 32 | U32, dtype=np.uint64)
    _lib.gpu_check(gm._g.kmpgpu_scan_headers(gm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_headers")
    assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))


@pytest.mark.parametrize("n_pkts", [129, 1000])
def test_rows_do_not_depend_on_the_text_rule_or_the_arena_route(gm, world, n_pkts):
    payloads, meta, heads, rows = world
    n_hdr = 65
    rows = rows[:n_hdr, :n_pkts]
    _not_trivial(rows)
    reset(gm)
    try:
        gm.set_patterns(PATS)
        load(gm, payloads[:n_pkts])
        gm.set_meta(meta[:n_pkts])
        gm.set_headers(heads[:n_hdr])
        for whole in (0, 1):                               # L_k is the index length whatever the text rule
            gm.set_option(OPT_WHOLE_PAYLOAD, whole)
            _check_headers(gm, rows)
        gm.set_option(OPT_WHOLE_PAYLOAD, 0)
        # a borrowed arena whose slots are not back to back, kept in place: the first marking pass packs it, and the metadata stays
        slots = [t + b"\xAA" * ((-len(t)) % 16 + 16) for t in payloads[:n_pkts]]
        gm.set_option(OPT_REPACK, 0)
        keep = attach_slots(gm, payloads[:n_pkts], slots)
        with raises(ESTATE, "no packet metadata"):         # the attach dropped it
            gm.scan_headers()
        gm.set_meta(meta[:n_pkts])
        _check_headers(gm, rows)
        assert gm.meta().tobytes() == meta[:n_pkts].tobytes()
        # ... and with the repack at the attach
        gm.set_option(OPT_REPACK, 1)
        keep = attach_slots(gm, payloads[:n_pkts], slots)
        gm.set_meta(meta[:n_pkts])
        _check_headers(gm, rows)
        del keep
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. as rule terms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel,fused", KERNELS)
@pytest.mark.parametrize("n_pkts", [130, N_MAX])
def test_headers_as_rule_terms(gm, world, oracle, n_pkts, name, kernel, fused):
    payloads, meta, heads, rows = world
    payloads, meta = payloads[:n_pkts], meta[:n_pkts]
    n_hdr = 16
    hrows = rows[:n_hdr, :n_pkts]
    _not_trivial(hrows)
    relations = [(0, 1, 0, 8), (2, 0, None, None)]
    chains = [(0, (1, 0, 4), (2, 0, None))]
    st = MM.starts(payloads, PATS)
    mat = np.concatenate([MM.hits(st, len(PATS)), MM.relation_rows(st, PATS, relations), CM.chain_rows(st, PATS, chains), hrows])
    np_, nr, nc = len(PATS), len(relations), len(chains)
    h0 = np_ + nr + nc
    rules = [([0, h0 + 0], []),                      # GET over udp
             ([1], [h0 + 1, h0 + 12]),               # /admin, not tcp, not empty
             ([np_ + 0, h0 + 4], [h0 + 0]),          # a relation from one /32 source, not over udp
             ([np_ + nr + 0, h0 + 5], [h0 + 3]),     # a chain, a /9 source, not to port 53
             ([h0 + 2, h0 + 13], [np_ + 1]),         # header terms and a negated relation
             ([], [h0 + 0, h0 + 1]),                 # negated header terms only: neither udp nor tcp -- the tail bits must stay 0
             ([], [h0 + 2]),                         # ... and nothing at all: not (any / any)
             ([h0 + 15, 0, 1, 2, h0 + 7], [h0 + 9, h0 + 12])]
    want = MM.rule_rows(mat, rules)
    assert 0 < want.sum() < want.size and want[5].any() and not want[6].any()
    reset(gm)
    try:
        gm.set_option(OPT_KERNEL, kernel)
        gm.set_option(OPT_FUSED, fused)
        gm.set_patterns(PATS)
        load(gm, payloads)
        gm.set_meta(meta)
        gm.set_relations(relations)
        gm.set_chains(chains)
        gm.set_headers(heads[:n_hdr])
        assert [gm.rel(0), gm.chain(0), gm.hdr(0), gm.hdr(15)] == [np_, np_ + nr, h0, h0 + 15]
        gm.set_rules(rules)
        counts = MM.oracle_counts(oracle, payloads, PATS)
        res = gm.scan_rules(hits=True)
        bad = np.argwhere(res["hits"] != want)
        assert bad.size == 0, [(int(r), int(k), bool(want[r, k])) for r, k in bad[:8]]
        assert res["rule_pkt_counts"].tolist() == want.sum(axis=1).tolist()
        assert res["any"].tolist() == want.any(axis=0).tolist()
        assert res["counts"].tolist() == counts
        # one launch more than the same rules' pass makes without the header kernel: relation, chain, header, rules kernels
        assert res["timing"].launches == gm.scan_packets()["timing"].launches - 1 + 4
        # the rules family is how header hits reach the alert list
        al = gm.scan_alerts("rules")
        assert [(int(a["packet"]), int(a["index"])) for a in al["alerts"]] == sorted((int(k), int(r)) for r, k in np.argwhere(want))
        assert al["n_found"] == int(want.sum()) and al["n_packets"] == int(want.any(axis=0).sum())
        assert al["timing"].launches == res["timing"].launches + 4
        # under a profile the header kernel is recorded between the chain kernel and the rules kernel: one entry more than without
        gm.profile_begin(64)
        gm.scan_rules()
        with_h = len(gm.profile_end(64))
        gm.set_headers([])
        gm.set_rules([([0], [1])])
        gm.profile_begin(64)
        gm.scan_rules()
        assert with_h == len(gm.profile_end(64)) + 1
        # the header rows themselves, behind relations and chains
        gm.set_headers(heads[:n_hdr])
        _check_headers(gm, hrows, counts)
    finally:
        reset(gm)


def test_alerts_have_no_header_family(gm, world):
    payloads, meta, heads, _ = world
    reset(gm)
    gm.set_patterns(PATS)
    load(gm, payloads[:64])
    gm.set_meta(meta[:64])
    gm.set_headers(heads[:3])
    found = _lib.C.c_uint64()
    assert gm._g.kmpgpu_scan_alerts(gm._ctx, 4, 10, _lib.C.byref(found), None, None, None, None) == EINVAL


# ------------------------------------------------------------------------------------------------
# 3. the metadata from the device's extraction
# ------------------------------------------------------------------------------------------------
def _synthetic_frames(n, mode):
    rng = np.random.default_rng(n)
    frames = []
    for i in range(n):
        f = HM.make_frame(mode, b"GET /admin %05d xyz" % i if i % 4 else b"", int(rng.choice(ADDR)), int(rng.choice(ADDR)), int(rng.choice(PORTS)),
                          int(rng.choice(PORTS)), ihl=(5, 6, 15, 5, 7)[i % 5], tcp_words=(5, 8)[i % 2])
        frames.append((20 if i % 3 == 2 else len(f), f))       # every third is cut short and rejected
    return frames


def _check_extraction(gm, path, mode):
    pay, meta = HM.capture(HM.pcap_frames(path), mode)
    host = HostArena.from_pcap(path, mode, with_meta=True)
    assert host.meta.tobytes() == meta.tobytes() and host.n_pkts == len(pay)
    gm.set_option(OPT_KEEP_META, 0)
    n0, _ = gm.load_pcap_frames(path, mode)
    assert n0 == len(pay)
    with raises(ESTATE, "no packet metadata"):
        gm.meta()
    plain = gm.arena_download() if n0 else None
    gm.set_option(OPT_KEEP_META, 1)
    n1, _ = gm.load_pcap_frames(path, mode)
    assert n1 == len(pay)
    got = gm.meta()
    assert got.dtype == META_DTYPE and got.tobytes() == meta.tobytes()
    if n1:
        for a, b in zip(plain, gm.arena_download()):           # the arena is the same either way, and the host's
            assert np.array_equal(a, b)
        assert np.array_equal(plain[2], host.len) and np.array_equal(plain[1], host.off)
    return pay, meta


@pytest.mark.parametrize("mode", ["udp", "tcp"])
def test_device_extraction_keeps_the_metadata_of_udp_1000(gm, mode):
    reset(gm)
    try:
        gm.set_patterns(PATS)
        pay, meta = _check_extraction(gm, os.path.join(DATA, "udp_1000.pcap"), mode)
        assert len(pay) == (321 if mode == "udp" else 20)
    finally:
        gm.set_option(OPT_KEEP_META, 0)


@pytest.mark.parametrize("mode", ["udp", "tcp"])
@pytest.mark.parametrize("n", [1, 64, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_device_extraction_keeps_the_metadata_of_synthetic_captures(gm, tmp_path, n, mode):
    path = str(tmp_path / "frames.pcap")
    HM.write_pcap(path, _synthetic_frames(n, mode))
    reset(gm)
    try:
        gm.set_patterns(PATS)
        pay, meta = _check_extraction(gm, path, mode)
        assert len(pay) == n - n // 3
        # and predicates over what the device extracted
        heads = _predicates(20)
        rows = HM.header_rows(meta, [len(t) for t in pay], heads)
        _not_trivial(rows)
        gm.set_headers(heads)
        _check_headers(gm, rows)
    finally:
        gm.set_option(OPT_KEEP_META, 0)


# ------------------------------------------------------------------------------------------------
# 4. lifecycle
# ------------------------------------------------------------------------------------------------
def test_set_calls_drop_and_keep(gm, world):
    payloads, meta, heads, rows = world
    n = 200
    reset(gm)
    gm.set_patterns(PATS)
    load(gm, payloads[:n])
    gm.set_meta(meta[:n])
    gm.set_rules([([0], [1])])
    before = gm.scan_rules(hits=True)
    # every successful kmpgpu_set_headers drops the rules
    gm.set_headers(heads[:5])
    with raises(ESTATE, "no rules set"):
        gm.scan_rules()
    gm.set_rules([([0, gm.hdr(0)], [gm.hdr(4)])])
    with_h = gm.scan_rules(hits=True)
    assert with_h["timing"].launches == before["timing"].launches + 1
    # kmpgpu_set_relations / _set_chains keep the headers and drop the rules
    gm.set_relations([(0, 1, None, None)])
    with raises(ESTATE, "no rules set"):
        gm.scan_rules()
    _check_headers(gm, rows[:5, :n])
    gm.set_chains([(0, (1, None, None))])
    _check_headers(gm, rows[:5, :n])
    assert gm.hdr(0) == len(PATS) + 2
    gm.set_rules([([gm.hdr(4)], [])])
    assert np.array_equal(gm.scan_rules(hits=True)["hits"][0], rows[4, :n])
    # errors keep the earlier state: predicates and rules
    bad = [dict(heads[0], sport_lo=5, sport_hi=4), dict(heads[0], dport_lo=9, dport_hi=8), dict(heads[0], len_lo=2, len_hi=1), dict(heads[0], flags=4)]
    for b in bad:
        with raises(EINVAL, "predicate 1"):
            gm.set_headers([heads[0], b])
    arr = np.zeros(1, dtype=gm.headers.dtype)
    arr["sport_hi"] = arr["dport_hi"] = 0xFFFF
    arr["len_hi"] = U32
    arr["reserved"] = 1
    with raises(EINVAL, "reserved is 1"):
        gm.set_headers(arr)
    assert gm._g.kmpgpu_set_headers(gm._ctx, None, 3) == EINVAL
    assert np.array_equal(gm.scan_rules(hits=True)["hits"][0], rows[4, :n])
    _check_headers(gm, rows[:5, :n])
    # n_hdr == 0 clears: the rules go, the rows are no terms any more, and scan_rules is what it was before any predicate was set
    gm.set_relations([])
    gm.set_chains([])
    gm.set_headers([])
    with raises(ESTATE, "no header predicates set"):
        gm.scan_headers()
    with raises(EINVAL, "names row 3"):
        gm.set_rules([([3], [])])
    gm.set_rules([([0], [1])])
    after = gm.scan_rules(hits=True)
    for key in ("hits", "rule_pkt_counts", "any", "counts"):
        assert np.array_equal(after[key], before[key]), key
    assert after["timing"].launches == before["timing"].launches
    # kmpgpu_set_patterns drops the headers with everything else; the metadata belongs to the arena and stays
    gm.set_headers(heads[:5])
    gm.set_patterns(PATS)
    with raises(ESTATE, "no header predicates set"):
        gm.scan_headers()
    assert gm.meta().tobytes() == meta[:n].tobytes()
    # no patterns: ESTATE
    with GpuMatcher(0) as m:
        with raises(ESTATE, "no patterns set"):
            m.set_headers(heads[:1])


def test_metadata_lifetime(gm, world):
    payloads, meta, heads, rows = world
    n = 300
    reset(gm)
    gm.set_patterns(PATS)
    gm.load_arena(HostArena.from_payloads([]))
    with raises(ESTATE, "no arena"):
        gm.set_meta(meta[:n])
    with raises(ESTATE, "no packet metadata"):
        gm.meta()
    load(gm, payloads[:n])
    gm.set_headers(heads[:4])
    gm.set_rules([([gm.hdr(0)], [])])
    # headers set, no metadata: all three calls refuse, and the context stays usable
    for call in (gm.scan_headers, gm.scan_rules, lambda: gm.scan_alerts("rules")):
        with raises(ESTATE, "no packet metadata"):
            call()
    assert gm.scan_packets()["counts"].tolist() == gm.scan()[0].tolist()
    # a wrong count, a NULL pointer, a bad flag: EINVAL, and what was there stays
    gm.set_meta(meta[:n])
    for wrong in (meta[:n - 1], meta[:n + 1]):
        with raises(EINVAL, f"{len(wrong)} records for the arena's {n} payloads"):
            gm.set_meta(wrong)
    assert gm._g.kmpgpu_set_meta(gm._ctx, None, n, 0) == EINVAL
    assert gm._g.kmpgpu_set_meta(gm._ctx, meta.ctypes.data, n, 2) == EINVAL
    assert gm.meta().tobytes() == meta[:n].tobytes()
    _check_headers(gm, rows[:4, :n])
    # from a device tensor
    shifted = np.roll(meta[:n], 1)
    t = torch.from_numpy(shifted.view(np.uint8).reshape(-1).copy()).cuda()
    gm.set_meta(t)
    assert gm.meta().tobytes() == shifted.tobytes()
    _check_headers(gm, HM.header_rows(shifted, [len(x) for x in payloads[:n]], heads[:4]))
    # options and set_patterns keep it; cleared by hand; dropped by every loader that brings a new arena
    gm.set_option(OPT_WHOLE_PAYLOAD, 1)
    gm.set_option(OPT_WHOLE_PAYLOAD, 0)
    assert gm.meta().tobytes() == shifted.tobytes()
    gm.set_meta(None)
    with raises(ESTATE, "no packet metadata"):
        gm.meta()
    gm.set_meta(meta[:n])
    load(gm, payloads[:n])
    with raises(ESTATE, "no packet metadata"):
        gm.meta()
    # an arena built with its metadata brings it along
    path = os.path.join(DATA, "udp_1000.pcap")
    host = HostArena.from_pcap(path, "udp", with_meta=True)
    gm.load_arena(host)
    assert gm.meta().tobytes() == host.meta.tobytes()
    gm.set_option(OPT_KEEP_META, 0)
    gm.load_pcap_frames(path, "udp")                       # without the option the load leaves none
    with raises(ESTATE, "no packet metadata"):
        gm.meta()
    with raises(EINVAL, "keep meta"):
        gm.set_option(OPT_KEEP_META, 2)


def test_no_payloads(gm, world):
    _, meta, heads, _ = world
    reset(gm)
    gm.set_patterns(PATS)
    gm.load_arena(HostArena.from_payloads([]))
    gm.set_meta(None)                                     # n_pkts == 0 with a NULL pointer: nothing to clear, no error
    gm.set_headers(heads[:3])
    res = gm.scan_headers(hits=True)
    assert res["hdr_pkt_counts"].tolist() == [0, 0, 0] and res["hits"].shape == (3, 0) and res["timing"].launches == 0
    gm.set_rules([([gm.hdr(1)], [])])
    assert gm.scan_rules()["rule_pkt_counts"].tolist() == [0]


# ------------------------------------------------------------------------------------------------
# 5. kmpgpu_load_selected
# ------------------------------------------------------------------------------------------------
def test_load_selected_hands_the_metadata_on(gm, world):
    payloads, meta, heads, rows = world
    n = 1500
    reset(gm)
    gm.set_patterns(PATS)
    load(gm, payloads[:n])
    select = rows[0, :n] | rows[12, :n]                   # udp, or empty
    assert 0 < select.sum() < n
    with GpuMatcher(0) as dst:
        # without metadata on src everything is as it was
        idx = dst.load_selected(gm, select)
        assert dst.last_timing().launches == 5
        with raises(ESTATE, "no packet metadata"):
            dst.meta()
        dst.load_selected(gm, np.zeros(n, dtype=bool))
        assert dst.last_timing().launches == 3
        # with it: the selected payloads' records, in order, by one kernel more
        gm.set_meta(meta[:n])
        idx = dst.load_selected(gm, select)
        assert idx.tolist() == np.flatnonzero(select).tolist()
        assert dst.last_timing().launches == 6
        assert dst.meta().tobytes() == meta[:n][idx.astype(np.int64)].tobytes()
        a, off, ln = dst.arena_download()
        assert ln.tolist() == [len(payloads[int(k)]) for k in idx]
        # the second stage: header rules over the compacted arena
        dst.set_patterns(PATS)
        dst.set_headers(heads[:16])
        sub = rows[:16, :n][:, idx.astype(np.int64)]
        _not_trivial(sub)
        _check_headers(dst, sub)
        dst.set_rules([([0, dst.hdr(0)], [dst.hdr(12)]), ([], [dst.hdr(0)])])
        hits = MM.hits(MM.starts([payloads[int(k)] for k in idx], PATS), len(PATS))
        want = MM.rule_rows(np.concatenate([hits, sub]), dst.rules)
        assert want[0].any() and want[1].any()
        assert np.array_equal(dst.scan_rules(hits=True)["hits"], want)
        # nothing selected: no arena, no metadata, four launches
        dst.load_selected(gm, np.zeros(n, dtype=bool))
        assert dst.last_timing().launches == 4 and dst.arena_info()[0] == 0
        with raises(ESTATE, "no packet metadata"):
            dst.meta()
    assert gm.meta().tobytes() == meta[:n].tobytes()     # src is not written


# ------------------------------------------------------------------------------------------------
# 6. the command lines: KMPGPU_HEADERS_FILE
# ------------------------------------------------------------------------------------------------
def _dotted(ip):
    return ".".join(str(ip >> s & 255) for s in (24, 16, 8, 0))


@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"])])
def test_cli_headers_file(tokens, tmp_path, prog, extra):
    pay, meta = HM.capture(HM.pcap_frames(os.path.join(DATA, "udp_1000.pcap")), "udp")
    lens = [len(t) for t in pay]
    n = len(tokens)
    ssdp, mdns_src = 0xEFFFFFFA, 0xC0A80000                # 239.255.255.250; 192.168.0.0/16
    heads = [H(proto=17, dport=(1900, 1900)), H(src=(mdns_src, 0xFFFF0000), sport=(5353, 5353), dst=(0xE00000FB, U32), bidir=True),
             H(proto=6), H(dst=(ssdp, U32), length=(0, 300)), H(sport=(1024, 65535), dport=(0, 1023), bidir=True, length=(40, U32))]
    hf = tmp_path / "headers.txt"
    hf.write_text("# proto src sport dir dst dport [len]\n"
                  "udp any any -> any 1900\n"
                  f"any {_dotted(mdns_src)}/16 5353 <> 224.0.0.251 5353:5353\n\n"
                  "tcp any any -> any any\n"
                  f"ip any any -> {_dotted(ssdp)}/32 any :300\n"
                  "any any 1024: <> any :1023 40:\n")
    hrows = HM.header_rows(meta, lens, heads)
    assert 0 < hrows.sum() < hrows.size and not hrows[2].any()
    hits = MM.hits(MM.starts(pay, tokens), n)
    busy = [int(i) for i in np.argsort(-hits.sum(axis=1))[:2]]
    rules = [([busy[0], n + 0], []), ([busy[1]], [n + 3]), ([n + 1], []), ([], [n + 2, n + 0]), ([n + 4], [n + 1])]
    want = MM.rule_rows(np.concatenate([hits, hrows]), rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size

    def term(i):
        return str(i) if i < n else f"h{i - n}"

    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([term(i) for i in pos] + ["!" + term(i) for i in neg]) + "\n" for pos, neg in rules))
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        golden = f.read()
    files = []
    for route in ("0", "1"):
        al = tmp_path / f"alerts{route}.csv"
        r = run_cli(prog, extra=extra, env_extra={"KMPGPU_HEADERS_FILE": str(hf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al),
                                                  "KMPGPU_DEVICE_EXTRACT": route})
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == golden
        files.append(al.read_bytes())
    got = [tuple(int(x) for x in line.split(",")) for line in files[0].decode().splitlines()]
    assert got == sorted((int(k), int(r_)) for r_, k in np.argwhere(want))
    assert files[0] == files[1]                            # host extraction and device extraction write the same bytes
