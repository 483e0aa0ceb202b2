"""kmpgpu_scan_thresholds past one level of tile aggregates: n = TILE^2 + TILE + 1 payloads, so the aggregates of both scans -- the running
maximum of the timestamps and the prefix sum of the hits -- are themselves more than one tile.  A periodic arena of 16-byte payloads laid
out on the device (tests/gpu_support.py); one tracker, 65 addresses and one flow; windows whose first payload lies in another tile, and
in another tile of aggregates, than the payload they end at.  Compared, exactly, against threshold_model.run_fast.
"""
import numpy as np
import pytest

from gpu_support import PERIOD, PeriodicSource, meta_of_flows, torch  # noqa: F401

import threshold_model as TM

pytestmark = pytest.mark.gpu

TILE = 256 * 4                # KMP_SCAN_TILE
N = TILE * TILE + TILE + 1
PATS = (b"AA", b"BB")
RULES = [([0], []), ([1], []), ([0], []), ([1], [])]
NEAR, FAR = 5 * TILE, 300 * TILE       # in the time of ts ~ 1.5 k: a few tiles back; further back than the last tile of aggregates is long


def payload(e):
    return (b"AA" if e % 4 == 1 else b"-") + (b"BB" if e % 3 == 0 else b"-") + b"%03d" % e


@pytest.fixture(scope="module")
def source():
    src = PeriodicSource(PATS)
    src.build([payload(e) for e in range(PERIOD)], N)
    src.m.set_rules(RULES)
    yield src
    src.close()


def times():
    """gaps of 0 to 3, and every 1000th payload steps far back: T differs from ts"""
    rng = np.random.default_rng(5)
    ts = np.cumsum(rng.integers(0, 4, N)).astype(np.uint64)
    ts[::1000] //= np.uint64(3)
    return ts


@pytest.mark.parametrize("shape", ["f65", "one"])
def test_two_levels_of_aggregates(source, shape):
    m = source.m
    k = np.arange(N)
    e = k % PERIOD
    aa, bb = e % 4 == 1, e % 3 == 0
    base = np.array([aa, bb, aa, bb])
    ts = times()
    flow = k % 65 if shape == "f65" else np.zeros(N, dtype=np.int64)
    meta = meta_of_flows(flow, seed=3)
    m.set_meta(meta)
    if shape == "f65":
        thr = [(0, "by_rule", "at_least", 850, NEAR), (1, "by_src", "at_most", 40, NEAR), (2, "by_src", "exactly", 1500, FAR),
               (3, "by_dst", "at_least", 100000, None), (3, "by_rule", "at_least", 30000, FAR)]
    else:
        assert m.build_flows() == 1
        thr = [(0, "by_flow", "at_least", 850, NEAR), (1, "by_flow", "at_most", 34000, FAR), (2, "by_rule", "exactly", 100000, None),
               (3, "by_flow", "at_least", 34000, FAR)]
    m.set_thresholds(thr)
    want = TM.run_fast(base, ts, thr, src=meta["src_ip"], dst=meta["dst_ip"], flow_of=flow)
    res = m.scan_thresholds(ts, hits=True, window_counts=True)
    for q in range(len(thr)):
        bad = np.flatnonzero(res["window_counts"][q] != want["window_counts"][q])
        assert bad.size == 0, (thr[q], bad[:8], want["window_counts"][q][bad[:8]], res["window_counts"][q][bad[:8]])
    for r in range(len(RULES)):
        assert np.array_equal(res["hits"][r], want["alert"][r]), (r, np.flatnonzero(res["hits"][r] != want["alert"][r])[:8])
    assert res["rule_pkt_counts"].tolist() == want["alert"].sum(axis=1).tolist()
    assert np.array_equal(res["any"], want["alert"].any(axis=0))
    assert res["counts"].tolist() == [int(aa.sum()), int(bb.sum())]
    # the cases are what the docstring says: every rule fires somewhere and not everywhere, and windows reach over tile borders
    for r in range(len(RULES)):
        assert 0 < want["alert"][r].sum() < base[r].sum(), (r, int(want["alert"][r].sum()))
    T = np.maximum.accumulate(ts)
    first = np.searchsorted(T, T - np.minimum(T, np.uint64(FAR)), side="right")       # (one tracker: the window's first payload)
    assert (first[TILE * TILE:] < TILE * TILE).all() and (k // TILE - first // TILE).max() > 64
