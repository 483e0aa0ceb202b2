"""kmpgpu_scan_flowbits past one level of tile aggregates: n = TILE^2 + TILE + 1 payloads, so the aggregates of the scan are themselves more
than one tile, as one flow and as flows of 3 payloads, whose heads fall on every position of a tile.  A periodic arena of 16-byte payloads
laid out on the device (tests/gpu_support.py) and op sets whose answer has a closed form in numpy -- fire once is the first hit of a
flow, a toggle is the parity of a prefix count -- on two levels.  Every comparison is exact.
"""
import numpy as np
import pytest

from gpu_support import PERIOD, PeriodicSource, meta_of_flows, torch  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = 256 * 4                # KMP_SCAN_TILE
N = TILE * TILE + TILE + 1
PATS = (b"AA", b"BB")
RULES = [([0], []), ([1], []), ([0], []), ([1], []), ([0], [])]
# bit 0: an AA was seen (rule 0 fires once); bit 1: the parity of the BBs (rule 1), tested by rule 2; bit 2, one level up: the parity of
# the BBs behind the first AA (rule 3), tested by rule 4
OPS = [(0, "isnotset", 0), (0, "set", 0), (1, "toggle", 1), (1, "noalert"), (2, "isset", 1), (3, "isset", 0), (3, "toggle", 2), (3, "noalert"),
       (4, "isset", 2)]


def payload(e):
    return (b"AA" if e % 4 == 1 else b"-") + (b"BB" if e % 3 == 0 else b"-") + b"%03d" % e


@pytest.fixture(scope="module")
def source():
    src = PeriodicSource(PATS)
    src.build([payload(e) for e in range(PERIOD)], N)
    src.m.set_rules(RULES)
    yield src
    src.close()


def before(events, start):
    """events of the payload's flow in front of it: start[k] is the flow's first payload"""
    c = np.concatenate([[0], np.cumsum(events)])
    return c[:-1] - c[start]


def total(events, start, last):
    """per flow, in the flows' order"""
    c = np.concatenate([[0], np.cumsum(events)])
    firsts = np.flatnonzero(np.arange(len(start)) == start)
    return c[last[firsts] + 1] - c[firsts]


@pytest.mark.parametrize("per_flow", [N, 3])
def test_two_levels_of_aggregates(source, per_flow):
    m = source.m
    k = np.arange(N)
    flow = k // per_flow
    start, last = flow * per_flow, np.minimum(flow * per_flow + per_flow - 1, N - 1)
    e = k % PERIOD
    aa, bb = e % 4 == 1, e % 3 == 0
    m.set_meta(meta_of_flows(flow, seed=per_flow))
    assert m.build_flows() == (N + per_flow - 1) // per_flow
    m.set_flowbits(OPS)
    res = m.scan_flowbits(hits=True, state=True)

    seen = before(aa, start) > 0
    odd = (before(bb, start) & 1) == 1
    behind = bb & seen
    odd2 = (before(behind, start) & 1) == 1
    for b, want in enumerate((seen, odd, odd2)):
        assert np.array_equal(res["state"][b], want), (b, np.flatnonzero(res["state"][b] != want)[:8])
    alert = [aa & ~seen, np.zeros(N, dtype=bool), aa & odd, np.zeros(N, dtype=bool), aa & odd2]
    for r, want in enumerate(alert):
        assert np.array_equal(res["hits"][r], want), (r, np.flatnonzero(res["hits"][r] != want)[:8])
    assert res["rule_pkt_counts"].tolist() == [int(a.sum()) for a in alert]
    assert np.array_equal(res["any"], alert[0] | alert[2] | alert[4])
    want_state = (total(aa, start, last) > 0) * 1 + (total(bb, start, last) & 1) * 2 + (total(behind, start, last) & 1) * 4
    assert np.array_equal(res["flow_state"], want_state.astype(np.uint32))
    assert res["counts"].tolist() == [int(aa.sum()), int(bb.sum())]
    # fire once is the first AA of every flow, and there is one in every flow of the single-flow shape
    assert int(alert[0].sum()) == int((total(aa, start, last) > 0).sum()) and (per_flow == 3 or int(alert[0].sum()) == 1)
