"""Rate thresholds on the GPU (kmpgpu_set_thresholds, kmpgpu_scan_thresholds; include/kmpgpu.h) against tests/threshold_model.py, the
definition as a sequential loop over a dict of trackers.  Every comparison is exact: alert rows, counts, any, the window counts of every
payload, and the raw words' bits at n_pkts and above.
"""
import os
import struct

import numpy as np
import pytest

from conftest import DATA

from gpu_support import EMPTY_ARENA, ONES, gm, load, meta_of_flows, reset, run_cli, strip_elapsed, torch  # noqa: F401  (gm: the context fixture)

import flow_model as FM
import match_model as MM
import threshold_model as TM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import HostArena
from multithreading_string_matching_amd.matcher import GpuMatcher

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
TILE = 256 * 4                # KMP_SCAN_TILE
SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
N_RULES = 8
PATS = [b"<%d>" % r for r in range(N_RULES)]           # rule r = pattern r: base[r][k] is bit r of the payload's mask
RULES = [([r], []) for r in range(N_RULES)]
MID = 700                     # with one tracker and ts = k: a window that starts in the middle of a tile, and in the tile before
# all four tracks, all three types, counts of 1 and above every run, windows 1 / MID / none, two thresholds on rule 3, none on rule 4
ALL = [(0, "by_src", "at_least", 2, MID), (1, "by_dst", "at_most", 1, 1), (2, "by_flow", "exactly", 2, None), (3, "by_rule", "at_least", 3, MID),
       (3, "by_src", "at_most", 5, None), (5, "by_flow", "at_least", 1 << 20, None), (6, "by_rule", "at_most", 1, 1), (7, "by_dst", "exactly", 1, MID)]


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


def masks_of(n, seed):
    """one 8-bit mask per payload: about a third of the payloads hold none of the patterns, the others one to three"""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=np.int64)
    for _ in range(3):
        m |= np.where(rng.integers(0, 3, n) == 0, 1 << rng.integers(0, N_RULES, n), 0)
    return m


def payloads_of(masks):
    return [b"".join(PATS[r] for r in range(N_RULES) if m >> r & 1) or b"-" for m in masks.tolist()]


def base_of(masks):
    return np.array([(masks >> r) & 1 for r in range(N_RULES)], dtype=bool)


def shapes(n):
    k = np.arange(n)
    out = {"one": np.zeros(n, dtype=np.int64), "each": k, "two": k % 2, "runs": (k + 32) // 64}
    for f in (63, 64, 65, 129):
        out[f"f{f}"] = k % f
    return out


def series(n, seed):
    """the time series: all equal, k, random gaps, one that steps back (T differs from ts), and values around 2^32, 2^63 and up to
    2^64 - 2, where only an unsigned 64-bit subtraction is right"""
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.uint64)
    gaps = np.cumsum(rng.integers(0, 2 * MID // 64 + 2, n)).astype(np.uint64)
    back = gaps.copy()
    back[rng.integers(0, 4, n) == 0] //= np.uint64(2)
    top = np.uint64((1 << 64) - 2)
    return {"equal": np.full(n, 5, dtype=np.uint64), "k": k, "gaps": gaps, "back": back,
            "b32": np.uint64((1 << 32) - n // 2) + k, "b63": np.uint64((1 << 63) - n // 2) + gaps,
            "b64": np.concatenate((gaps[:n // 2], top - gaps[:n - n // 2][::-1]))}


def setup(gm, masks):
    reset(gm)
    gm.set_patterns(PATS)
    gm.set_rules(RULES)
    load(gm, payloads_of(masks))


def check(gm, base, ts, thr, meta=None, fo=None, raw=False):
    keys = {"flow_of": fo}
    if meta is not None:
        keys.update(src=meta["src_ip"], dst=meta["dst_ip"])
    want = TM.run(base, ts, thr, **keys)
    res = gm.scan_thresholds(ts, hits=True, window_counts=True)
    bad = np.argwhere(res["window_counts"] != want["window_counts"])
    assert bad.size == 0, [(thr[q], int(k), int(want["window_counts"][q, k]), int(res["window_counts"][q, k])) for q, k in bad[:8]]
    bad = np.argwhere(res["hits"] != want["alert"])
    assert bad.size == 0, [(int(r), int(k), bool(want["alert"][r, k])) for r, k in bad[:8]]
    assert res["window_counts"].dtype == np.uint32
    assert res["rule_pkt_counts"].tolist() == want["alert"].sum(axis=1).tolist()
    assert res["any"].tolist() == want["alert"].any(axis=0).tolist()
    assert res["counts"].tolist() == base.sum(axis=1).tolist()         # (no pattern overlaps another or itself)
    # without the window counts a payload that does not hit skips the search: the same rows
    lean = gm.scan_thresholds(ts, hits=True)
    assert np.array_equal(lean["hits"], want["alert"]) and lean["rule_pkt_counts"].tolist() == res["rule_pkt_counts"].tolist()
    if raw:
        # the raw words: the bits at n_pkts and above are 0 in every word
        n = base.shape[1]
        W = (n + 63) // 64
        hit_w, any_w = np.full((N_RULES, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
        t64 = np.ascontiguousarray(ts, dtype=np.uint64)
        _lib.gpu_check(gm._g.kmpgpu_scan_thresholds(gm._ctx, t64.ctypes.data, 0, None, any_w.ctypes.data, hit_w.ctypes.data, None, None, None),
                       "kmpgpu_scan_thresholds")
        assert np.array_equal(hit_w, MM.words(want["alert"])) and np.array_equal(any_w, MM.words(want["alert"].any(axis=0)))
    return res, want


# ------------------------------------------------------------------------------------------------
# 1. payload counts x tracker shapes x time series
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_shapes(gm, n):
    masks = masks_of(n, n)
    base = base_of(masks)
    setup(gm, masks)
    times = series(n, n)
    names = list(times)
    for i, (name, flow) in enumerate(shapes(n).items()):
        meta = meta_of_flows(flow, seed=n)
        gm.set_meta(meta)
        assert gm.build_flows() == len(set(flow.tolist()))
        assert np.array_equal(gm.flow_ids(), flow), name
        gm.set_thresholds(ALL)                         # (the flows' rebuild keeps the thresholds: set once more only to say so)
        which = names[(i + n) % len(names)]
        _, want = check(gm, base, times[which], ALL, meta, flow, raw=name in ("one", "f65"))
        assert np.array_equal(want["alert"][4], base[4]) and not want["alert"][5].any(), (name, which)


@pytest.mark.parametrize("n", [257, 2 * TILE + 1])
def test_every_time_series_and_window(gm, n):
    masks = masks_of(n, n + 3)
    base = base_of(masks)
    setup(gm, masks)
    flow = np.arange(n) % 3
    meta = meta_of_flows(flow, seed=5)
    gm.set_meta(meta)
    gm.build_flows()
    seen = 0
    for name, ts in series(n, n + 1).items():
        assert (not np.array_equal(np.maximum.accumulate(ts), ts)) == (name == "back")
        for window in (1, MID, None):
            thr = [(r, TM.TRACKS[(r + seen) % 4], TM.TYPES[(r + seen // 4) % 3], 1 + (r * 3 + seen) % 5, window) for r in range(N_RULES) if r != 4]
            gm.set_thresholds(thr)
            _, want = check(gm, base, ts, thr, meta, flow, raw=seen % 7 == 0)
            seen += 1
            # a window of MID holds more than one payload somewhere, and fewer than all of them
            if window == MID and n > MID and name in ("k", "gaps", "b32", "b63"):
                wc = want["window_counts"]
                assert wc.max() > 1 and any(wc[q].max() < base[t[0]].sum() for q, t in enumerate(thr) if t[1] == "by_rule")


def test_directed_flows_and_a_second_arena(gm):
    n = TILE + 1
    masks = masks_of(n, 7)
    base = base_of(masks)
    setup(gm, masks)
    ts = series(n, 3)["gaps"]
    flow = np.arange(n) % 65
    meta = meta_of_flows(flow, seed=3)
    gm.set_meta(meta)
    gm.build_flows()
    gm.set_thresholds(ALL)
    _, undirected = check(gm, base, ts, ALL, meta, FM.flow_of(meta))
    # directed: the answers of a flow are a flow, and a tracker, of their own; build_flows keeps the thresholds
    assert gm.build_flows(directed=True) > 65
    _, directed = check(gm, base, ts, ALL, meta, FM.flow_of(meta, directed=True))
    assert not np.array_equal(undirected["window_counts"], directed["window_counts"])
    gm.build_flows()
    check(gm, base, ts, ALL, meta, FM.flow_of(meta))
    # other metadata: other flows, and other address orders
    flow2 = (np.arange(n) + 32) // 64
    meta2 = meta_of_flows(flow2, seed=4)
    gm.set_meta(meta2)
    with raises(ESTATE, "no flows"):
        gm.scan_thresholds(ts)
    by_addr = [t for t in ALL if t[1] != "by_flow"]
    gm.set_thresholds(by_addr)                         # without a by_flow threshold no flows are needed
    _, second = check(gm, base, ts, by_addr, meta2)
    assert not np.array_equal(second["window_counts"][0], undirected["window_counts"][0])
    gm.set_thresholds(ALL)
    gm.build_flows()
    check(gm, base, ts, ALL, meta2, flow2)
    # a second arena with other payloads and other addresses
    masks3 = masks_of(n - 70, 8)
    load(gm, payloads_of(masks3))
    meta3 = meta_of_flows(np.arange(n - 70) % 7, seed=9)
    gm.set_meta(meta3)
    gm.build_flows()
    check(gm, base_of(masks3), ts[:n - 70], ALL, meta3, FM.flow_of(meta3), raw=True)


def test_ts_as_a_device_tensor_is_ts_from_the_host(gm):
    n = 2 * TILE + 1
    masks = masks_of(n, 21)
    base = base_of(masks)
    setup(gm, masks)
    meta = meta_of_flows(np.arange(n) % 129, seed=2)
    gm.set_meta(meta)
    gm.build_flows()
    gm.set_thresholds(ALL)
    for name in ("back", "b64"):
        ts = series(n, 4)[name]
        host = gm.scan_thresholds(ts, hits=True, window_counts=True)
        # 8-byte aligned and no more: one element into a tensor
        dev = torch.from_numpy(np.concatenate(([0], ts.view(np.int64)))).cuda()[1:]
        assert dev.data_ptr() % 16 == 8
        got = gm.scan_thresholds(dev, hits=True, window_counts=True)
        assert np.array_equal(got["hits"], host["hits"]) and np.array_equal(got["window_counts"], host["window_counts"])
        assert np.array_equal(got["hits"], TM.run(base, ts, ALL, src=meta["src_ip"], dst=meta["dst_ip"], flow_of=FM.flow_of(meta))["alert"])
        assert np.array_equal(gm.scan_thresholds(torch.from_numpy(ts.view(np.int64)), hits=True)["hits"], host["hits"])     # a host tensor
    with pytest.raises(ValueError):
        gm.scan_thresholds(ts[:-1])
    with pytest.raises(ValueError):
        gm.scan_thresholds(torch.zeros(n, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------
# 2. states and errors
# ------------------------------------------------------------------------------------------------
def _set_raw(gm, rows):
    arr = (_lib.Threshold * max(len(rows), 1))()
    for a, (rule, track, typ, count, window) in zip(arr, rows):
        a.rule, a.track, a.type, a.count, a.window = rule, track, typ, count, window
    _lib.gpu_check(gm._g.kmpgpu_set_thresholds(gm._ctx, arr, len(rows)), "kmpgpu_set_thresholds")


def _scan_raw(gm, ts, on_device):
    _lib.gpu_check(gm._g.kmpgpu_scan_thresholds(gm._ctx, ts, on_device, None, None, None, None, None, None), "kmpgpu_scan_thresholds")


def test_states_and_errors(gm):
    n = 130
    masks = masks_of(n, 5)
    base = base_of(masks)
    flow = np.arange(n) % 3
    ts = np.arange(n, dtype=np.uint64) * np.uint64(3)
    by_rule = [(0, "by_rule", "at_least", 2, 10)]
    m = GpuMatcher(0)
    try:
        with raises(ESTATE, "no patterns set"):
            m.set_thresholds(by_rule)
        m.set_patterns(PATS)
        with raises(ESTATE, "kmpgpu_set_thresholds: no rules set"):
            m.set_thresholds(by_rule)
        with raises(ESTATE, "kmpgpu_scan_thresholds: no rules set"):
            m.scan_thresholds(np.zeros(0, np.uint64))
        m.set_rules(RULES)
        with raises(ESTATE, "no thresholds"):
            m.scan_thresholds(np.zeros(0, np.uint64))
        m.set_thresholds(by_rule)
        with raises(ESTATE, "kmpgpu_scan_thresholds: no arena loaded"):         # patterns, rules and thresholds, and no load call yet
            m.scan_thresholds(np.zeros(0, np.uint64))
        with raises(ESTATE, "kmpgpu_scan_thresholds: no arena loaded"):
            _scan_raw(m, None, 0)
        # an empty arena: everything is 0 and nothing is launched
        m.load_arena(*EMPTY_ARENA)
        res = m.scan_thresholds(np.zeros(0, np.uint64), hits=True, window_counts=True)
        assert res["rule_pkt_counts"].tolist() == [0] * N_RULES and res["counts"].tolist() == [0] * N_RULES and res["timing"].launches == 0
        assert res["hits"].shape == (N_RULES, 0) and res["window_counts"].shape == (1, 0)
        _scan_raw(m, None, 0)                             # (no timestamps for no payloads)
        load(m, payloads_of(masks))
        check(m, base, ts, by_rule)                       # by_rule needs neither metadata nor flows
        with raises(EINVAL, "ts is NULL"):
            _scan_raw(m, None, 0)
        for bad in (2, -1):
            with raises(EINVAL, f"ts_on_device is {bad}, not 0 or 1"):
                _scan_raw(m, ts.ctypes.data, bad)
        # device timestamps at an address that is 4 mod 8
        odd = torch.zeros(2 * n + 1, dtype=torch.int32, device="cuda")[1:]
        assert odd.data_ptr() % 8 == 4
        with raises(EINVAL, "the device timestamps are not 8-byte aligned"):
            _scan_raw(m, odd.data_ptr(), 1)
        check(m, base, ts, by_rule)
        # numpy timestamps that are no non-negative integers are refused by the Python layer
        for bad_ts in (ts.astype(np.float64), -ts.astype(np.int64) - 1):
            with pytest.raises(ValueError):
                m.scan_thresholds(bad_ts)
        m.set_thresholds([(0, "by_src", "at_least", 2, 10)])
        with raises(ESTATE, "no packet metadata"):
            m.scan_thresholds(ts)
        m.set_thresholds([(0, "by_dst", "at_least", 2, 10)])
        with raises(ESTATE, "no packet metadata"):
            m.scan_thresholds(ts)
        m.set_thresholds([(0, "by_flow", "at_least", 2, 10)])
        with raises(ESTATE, "no flows"):
            m.scan_thresholds(ts)
        meta = meta_of_flows(flow)
        m.set_meta(meta)
        with raises(ESTATE, "no flows"):
            m.scan_thresholds(ts)
        m.build_flows()
        m.set_thresholds(ALL)
        check(m, base, ts, ALL, meta, flow)
        # every refusal leaves the thresholds before it in force
        NOW = _lib.THR_NO_WINDOW
        for rows, text in [([(N_RULES, 0, 0, 1, NOW)], f"threshold 0 names rule {N_RULES} of {N_RULES}"),
                           ([(0, 0, 0, 1, NOW), (0, 4, 0, 1, NOW)], "threshold 1: track 4 is none of KMPGPU_THR_BY_"),
                           ([(0, 0, 3, 1, NOW)], "threshold 0: type 3 is none of KMPGPU_THR_AT_LEAST"),
                           ([(0, 0, 0, 0, NOW)], "threshold 0: count is 0"), ([(0, 0, 0, 1, 0)], "threshold 0: window is 0")]:
            with raises(EINVAL, text):
                _set_raw(m, rows)
            check(m, base, ts, ALL, meta, flow)
        with raises(EINVAL, "thr is NULL"):
            _lib.gpu_check(m._g.kmpgpu_set_thresholds(m._ctx, None, 1), "kmpgpu_set_thresholds")
        check(m, base, ts, ALL, meta, flow)
        # clearing; new rules drop the thresholds, and so do new patterns; build_flows keeps them
        m.set_thresholds([])
        with raises(ESTATE, "no thresholds"):
            m.scan_thresholds(ts)
        m.set_thresholds(ALL)
        m.build_flows()
        check(m, base, ts, ALL, meta, flow)
        m.set_rules(RULES)
        assert m.thresholds == []
        with raises(ESTATE, "no thresholds"):
            m.scan_thresholds(ts)
        m.set_thresholds(ALL)
        m.set_patterns(PATS)
        with raises(ESTATE, "no rules set"):
            m.scan_thresholds(ts)
        # the Python layer's own checks
        for bad in ([(0, "by_pair", "at_least", 1, 1)], [(0, "by_src", "at_last", 1, 1)], [(0, "by_src", "at_least", 1)], [(0,)]):
            with pytest.raises(ValueError):
                m.set_thresholds(bad)
    finally:
        m.close()


def test_between_load_frames_begin_and_finish(gm):
    arena = HostArena.from_pcap(os.path.join(DATA, "udp.pcap"), "udp")
    file_bytes = np.fromfile(os.path.join(DATA, "udp.pcap"), dtype=np.uint8)
    m = GpuMatcher(0)
    try:
        m.set_patterns(PATS)
        m.set_rules(RULES)
        m.set_thresholds([(0, "by_rule", "at_least", 1, None)])
        G = _lib.gpu_lib()
        # one frame of the capture: its record's data starts behind the 24-byte file header and the 16-byte record header
        caplen = struct.unpack_from("<I", file_bytes.tobytes(), 24 + 8)[0]
        off, cl = np.array([40], dtype=np.uint64), np.array([caplen], dtype=np.uint32)
        n_pkts = _lib.C.c_uint64()
        _lib.gpu_check(G.kmpgpu_load_frames_begin(m._ctx, file_bytes.ctypes.data_as(_lib.u8p), file_bytes.size, off.ctypes.data_as(_lib.u64p),
                                                  cl.ctypes.data_as(_lib.u32p), 1, 0), "kmpgpu_load_frames_begin")
        one = np.zeros(1, np.uint64)
        with raises(ESTATE, "between kmpgpu_load_frames_begin and _finish"):
            _scan_raw(m, one.ctypes.data, 0)
        _lib.gpu_check(G.kmpgpu_load_frames_uploaded(m._ctx), "kmpgpu_load_frames_uploaded")
        _lib.gpu_check(G.kmpgpu_load_frames_finish(m._ctx, _lib.C.byref(n_pkts)), "kmpgpu_load_frames_finish")
        assert n_pkts.value == 1 and arena.n_pkts >= 1
        assert m.scan_thresholds(one, hits=True)["hits"].shape == (N_RULES, 1)      # ... and behind _finish the call is served
    finally:
        m.close()


def test_the_other_calls_are_what_they_were(gm):
    """scan_rules, scan_flowbits and scan_flows give the same bits and the same launches before and after the threshold calls"""
    n = TILE + 1
    masks = masks_of(n, 13)
    flow = np.arange(n) % 64
    ts = series(n, 2)["gaps"]
    fb = [(0, "isnotset", 0), (0, "set", 0), (2, "isset", 0)]

    def snapshot():
        rules = gm.scan_rules(hits=True)
        bits = gm.scan_flowbits(hits=True, state=True)
        folded = gm.scan_flows("rules", "flow", hits=True)
        return (rules["hits"].tobytes(), rules["rule_pkt_counts"].tobytes(), rules["any"].tobytes(), rules["timing"].launches,
                bits["hits"].tobytes(), bits["state"].tobytes(), bits["flow_state"].tobytes(), bits["timing"].launches,
                folded["hits"].tobytes(), folded["flow_counts"].tobytes(), folded["timing"].launches)
    setup(gm, masks)
    gm.set_meta(meta_of_flows(flow, seed=2))
    gm.build_flows()
    gm.set_flowbits(fb)
    gm.scan_flowbits()                                 # (the flows' order is built by the first call and kept)
    before = snapshot()
    gm.set_thresholds(ALL)
    gm.scan_thresholds(ts, hits=True, window_counts=True)
    assert snapshot() == before
    gm.scan_thresholds(ts)
    gm.set_thresholds([])
    assert snapshot() == before
    # the flows' order is one: whoever comes first builds it, the other finds it
    gm.build_flows()
    gm.set_thresholds([(0, "by_flow", "at_least", 2, None)])
    first = gm.scan_thresholds(ts)["timing"].launches
    assert gm.scan_thresholds(ts)["timing"].launches == first - 2
    assert gm.scan_flowbits()["timing"].launches == before[7]


# ------------------------------------------------------------------------------------------------
# 3. the command line
# ------------------------------------------------------------------------------------------------
def pcap_times(path):
    """the records' ts_sec * 1e6 + ts_usec of a classic little-endian microsecond capture, read here"""
    b = open(path, "rb").read()
    assert b[:4] == bytes.fromhex("d4c3b2a1")
    out, pos = [], 24
    while pos < len(b):
        sec, usec, caplen, _ = struct.unpack_from("<IIII", b, pos)
        out.append(sec * 1_000_000 + usec)
        pos += 16 + caplen
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"])])
def test_cli_on_a_tcp_capture(tmp_path, prog, extra):
    """tests/golden/data/tcp.pcap: one conversation of 13 segments, four of them a GET 0.4, 0.4 and 0.8 s apart"""
    path = os.path.join(DATA, "tcp.pcap")
    arena = HostArena.from_pcap(path, "tcp", with_meta=True, with_ts=True)
    ts = pcap_times(path)
    assert arena.n_pkts == len(ts) == 13 and np.array_equal(arena.ts, ts)            # (the tcp extractor accepts every frame of it)
    payloads = [bytes(arena.bytes[int(o):int(o) + int(ln)]) for o, ln in zip(arena.off, arena.len)]
    pats = [b"GET", b"204", b"Host:"]
    hits = MM.hits(MM.starts(payloads, pats), len(pats))
    assert hits[0].sum() == 4 and hits[1].any()
    rules = [([0, 2], []), ([1], []), ([0], [])]
    base = MM.rule_rows(hits, rules)
    strings, rules_f, thr_f, alerts = (tmp_path / name for name in ("strings.txt", "rules.txt", "thresholds.txt", "alerts.csv"))
    strings.write_bytes(b"\n".join(pats) + b"\n")
    rules_f.write_text("0 2\n1\n0\n")
    thr_f.write_text("# the first request of a connection; a second request within half a second\n0 by_flow at_most 1 all\n\n2 by_src at_least 2 0.5\n")
    thr = [(0, "by_flow", "at_most", 1, None), (2, "by_src", "at_least", 2, 500_000)]
    plain = run_cli(prog, "tcp.pcap", str(strings), extra, mode="tcp")
    assert plain.returncode == 0, plain.stderr
    for directed in (False, True):
        env = {"KMPGPU_RULES_FILE": str(rules_f), "KMPGPU_ALERTS_FILE": str(alerts), "KMPGPU_THRESHOLDS_FILE": str(thr_f)}
        if directed:
            env["KMPGPU_FLOWS_DIRECTED"] = "1"
        r = run_cli(prog, "tcp.pcap", str(strings), extra, env_extra=env, mode="tcp")
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == strip_elapsed(plain.stdout)
        want = TM.run(base, ts, thr, src=arena.meta["src_ip"], dst=arena.meta["dst_ip"], flow_of=FM.flow_of(arena.meta, directed))["alert"]
        # the first GET alone; the second and the third GET, which follow one within half a second; the answer as it is
        assert want[0].sum() == 1 and want[2].sum() == 2 and np.array_equal(want[1], base[1])
        assert alerts.read_text() == "".join(f"{k},{r}\n" for k, r in sorted((int(k), int(r)) for r, k in np.argwhere(want)))
