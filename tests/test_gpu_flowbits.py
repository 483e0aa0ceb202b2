"""Flow bits on the GPU (kmpgpu_set_flowbits, kmpgpu_scan_flowbits; include/kmpgpu.h) against tests/flowbit_model.py, the definition as a
sequential loop over a dict of flows.  Every comparison is exact: alert rows, counts, any, the before rows of every bit, the flows' last
states, and the raw words' bits at n_pkts and above.
"""
import os

import numpy as np
import pytest

from conftest import DATA

from gpu_support import EMPTY_ARENA, ONES, gm, load, meta_of_flows, reset, run_cli, strip_elapsed, torch  # noqa: F401  (gm: the context fixture)

import flow_model as FM
import flowbit_model as FB
import match_model as MM
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
# fire once (rule 0), a login that does not alert (1), the command behind it (2), the logout (3); rule 4 has no op
SESSION = [(0, "isnotset", 0), (0, "set", 0), (1, "set", 1), (1, "noalert"), (2, "isset", 1), (3, "unset", 1), (3, "noalert")]


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


def setup(gm, masks):
    reset(gm)
    gm.set_patterns(PATS)
    gm.set_rules(RULES)
    load(gm, payloads_of(masks))


def check(gm, base, fo, ops, n_bits, raw=True):
    want = FB.run(base, fo, ops, n_bits)
    res = gm.scan_flowbits(hits=True, state=True)
    bad = np.argwhere(res["hits"] != want["alert"])
    assert bad.size == 0, [(int(r), int(k), bool(want["alert"][r, k])) for r, k in bad[:8]]
    bad = np.argwhere(res["state"] != want["state"])
    assert bad.size == 0, [(int(b), int(k), bool(want["state"][b, k])) for b, k in bad[:8]]
    assert res["rule_pkt_counts"].tolist() == want["alert"].sum(axis=1).tolist()
    assert res["any"].tolist() == want["alert"].any(axis=0).tolist()
    assert res["flow_state"].dtype == np.uint32 and res["flow_state"].tolist() == want["flow_state"].tolist()
    assert res["counts"].tolist() == base.sum(axis=1).tolist()         # (no pattern overlaps another or itself)
    if raw:
        # the raw words: the bits at n_pkts and above are 0 in every word
        n = base.shape[1]
        W = (n + 63) // 64
        hit_w, st_w, any_w = np.full((N_RULES, W), ONES, dtype=np.uint64), np.full((n_bits, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
        _lib.gpu_check(gm._g.kmpgpu_scan_flowbits(gm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, st_w.ctypes.data, None, None, None),
                       "kmpgpu_scan_flowbits")
        assert np.array_equal(hit_w, MM.words(want["alert"])) and np.array_equal(st_w, MM.words(want["state"]))
        assert np.array_equal(any_w, MM.words(want["alert"].any(axis=0)))
    return res, want


# ------------------------------------------------------------------------------------------------
# 1. payload counts x flow shapes: fire once, a gate and an unset
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_shapes(gm, n):
    masks = masks_of(n, n)
    base = base_of(masks)
    setup(gm, masks)
    for name, flow in shapes(n).items():
        gm.set_meta(meta_of_flows(flow, seed=n))
        assert gm.build_flows() == len(set(flow.tolist()))
        assert np.array_equal(gm.flow_ids(), flow), name
        gm.set_flowbits(SESSION)                       # (the flows' rebuild keeps the ops: set once more only to say so)
        _, want = check(gm, base, flow, SESSION, 2, raw=name in ("one", "f65"))
        # fire once is the first base hit of every flow
        first = np.zeros(n, dtype=bool)
        seen = set()
        for k in np.flatnonzero(base[0]).tolist():
            if flow[k] not in seen:
                seen.add(flow[k])
                first[k] = True
        assert np.array_equal(want["alert"][0], first) and not want["alert"][1].any() and np.array_equal(want["alert"][4], base[4])


def test_rebuilding_the_flows_keeps_the_ops_and_renews_the_order(gm):
    n = TILE + 1
    masks = masks_of(n, 7)
    base = base_of(masks)
    setup(gm, masks)
    flow = np.arange(n) % 65
    meta = meta_of_flows(flow, seed=3)
    gm.set_meta(meta)
    gm.build_flows()
    gm.set_flowbits(SESSION)
    _, undirected = check(gm, base, FM.flow_of(meta), SESSION, 2)
    # directed: the answers of a flow are a flow, and a state, of their own
    assert gm.build_flows(directed=True) > 65
    _, directed = check(gm, base, FM.flow_of(meta, directed=True), SESSION, 2)
    assert not np.array_equal(undirected["alert"], directed["alert"])
    gm.build_flows()
    check(gm, base, FM.flow_of(meta), SESSION, 2)
    # other metadata: other flows
    flow2 = (np.arange(n) + 32) // 64
    gm.set_meta(meta_of_flows(flow2, seed=4))
    with raises(ESTATE, "no flows"):
        gm.scan_flowbits()
    gm.build_flows()
    check(gm, base, flow2, SESSION, 2)


# ------------------------------------------------------------------------------------------------
# 2. random op sets
# ------------------------------------------------------------------------------------------------
def random_ops(rng):
    """8 rules over 1..32 bits on up to four levels: a rule acts on bits of its level and above and tests bits below it, and the bit it
    acts on where that is one bit (a self-loop); acyclic by construction"""
    n_bits = int(rng.integers(1, 33))
    level = rng.integers(0, 4, n_bits)
    ops = []
    # every other set with four bits or more: rules 0, 1, 2 are a chain through one bit of every level, so the fourth level is reached
    chain = rng.choice(n_bits, size=4, replace=False).tolist() if n_bits >= 4 and rng.integers(0, 2) else []
    for j, b in enumerate(chain):
        level[b] = j
    for r in range(N_RULES):
        if chain and r < 3:
            ops += [(r, ("isset", "isnotset")[int(rng.integers(0, 2))], int(chain[r])), (r, ("set", "toggle")[int(rng.integers(0, 2))], int(chain[r + 1]))]
            continue
        if rng.integers(0, 8) == 0:
            continue                                   # a rule without ops
        if rng.integers(0, 4) == 0:
            ops.append((r, "noalert"))
        L = int(rng.integers(0, 4))
        above = np.flatnonzero(level >= L)
        below = np.flatnonzero(level < L)
        acted = rng.choice(above, size=min(len(above), int(rng.integers(0, 3))), replace=False).tolist() if len(above) else []
        tested = rng.choice(below, size=min(len(below), int(rng.integers(0, 3))), replace=False).tolist() if len(below) else []
        if len(acted) == 1 and rng.integers(0, 2):
            tested.append(acted[0])
        mine = [(r, ("isset", "isnotset")[int(rng.integers(0, 2))], int(b)) for b in tested]
        for b in acted:
            for _ in range(int(rng.integers(1, 3))):
                mine.append((r, ("set", "unset", "toggle")[int(rng.integers(0, 3))], int(b)))
        ops += [mine[i] for i in rng.permutation(len(mine))] if mine else []
    return ops, n_bits


@pytest.mark.parametrize("n", [257, TILE + 1])
def test_random_op_sets(gm, n):
    rng = np.random.default_rng(n)
    masks = masks_of(n, n + 1)
    base = base_of(masks)
    setup(gm, masks)
    flows = [np.arange(n) % 5, rng.integers(0, 40, n), np.zeros(n, dtype=np.int64)]
    orders, deepest, loops = [], 0, 0
    for i in range(200):
        if i % 67 == 0:
            flow = flows[i // 67]
            _, flow = np.unique(flow, return_inverse=True)                     # dense numbers, which are not yet in order of appearance
            firsts = {}
            flow = np.array([firsts.setdefault(int(f), len(firsts)) for f in flow])
            gm.set_meta(meta_of_flows(flow, seed=i))
            gm.build_flows()
            assert np.array_equal(gm.flow_ids(), flow)
        ops, n_bits = random_ops(rng)
        if not ops:
            continue
        lv = FB.levels(ops, n_bits)
        assert lv is not None
        deepest = max(deepest, max(lv))
        loops += any(a[0] == b[0] and a[2] == b[2] for a in ops for b in ops if a[1] in FB.TESTS and b[1] in FB.ACTIONS)
        gm.set_flowbits(ops, n_bits)
        check(gm, base, flow, ops, n_bits, raw=i % 20 == 0)
    assert deepest == 3 and loops > 20                 # four levels and self-loops were among them


def test_an_empty_effect_is_scan_rules(gm):
    n = 2 * TILE + 1
    masks = masks_of(n, 11)
    setup(gm, masks)
    gm.set_meta(meta_of_flows(np.arange(n) % 129, seed=1))
    gm.build_flows()
    plain = gm.scan_rules(hits=True)
    gm.set_flowbits([(3, "set", 5), (0, "toggle", 5), (7, "unset", 5)], n_bits=6)    # nobody tests bit 5
    res = gm.scan_flowbits(hits=True, state=True)
    assert np.array_equal(res["hits"], plain["hits"]) and res["rule_pkt_counts"].tolist() == plain["rule_pkt_counts"].tolist()
    assert res["any"].tolist() == plain["any"].tolist() and res["counts"].tolist() == plain["counts"].tolist()
    assert res["state"][5].any() and not res["state"][:5].any()


# ------------------------------------------------------------------------------------------------
# 3. states and errors
# ------------------------------------------------------------------------------------------------
def _set_raw(gm, rows, n_bits):
    arr = (_lib.FlowbitOp * max(len(rows), 1))()
    for a, (rule, bit, op, reserved) in zip(arr, rows):
        a.rule, a.bit, a.op, a.reserved = rule, bit, op, reserved
    _lib.gpu_check(gm._g.kmpgpu_set_flowbits(gm._ctx, arr, len(rows), n_bits), "kmpgpu_set_flowbits")


def test_states_and_errors(gm):
    n = 130
    masks = masks_of(n, 5)
    base = base_of(masks)
    flow = np.arange(n) % 3
    m = GpuMatcher(0)
    try:
        with raises(ESTATE, "no patterns set"):
            m.set_flowbits([(0, "set", 0)])
        m.set_patterns(PATS)
        with raises(ESTATE, "kmpgpu_set_flowbits: no rules set"):
            m.set_flowbits([(0, "set", 0)])
        with raises(ESTATE, "kmpgpu_scan_flowbits: no rules set"):
            m.scan_flowbits()
        m.set_rules(RULES)
        with raises(ESTATE, "no flow bits"):
            m.scan_flowbits()
        m.set_flowbits(SESSION)
        with raises(ESTATE, "no flows"):
            m.scan_flowbits()
        # an empty arena: everything is 0 and nothing is launched
        m.load_arena(*EMPTY_ARENA)
        m.build_flows()
        res = m.scan_flowbits(hits=True, state=True)
        assert res["rule_pkt_counts"].tolist() == [0] * N_RULES and res["counts"].tolist() == [0] * N_RULES and res["timing"].launches == 0
        assert res["hits"].shape == (N_RULES, 0) and res["state"].shape == (2, 0) and len(res["flow_state"]) == 0
        load(m, payloads_of(masks))
        with raises(ESTATE, "no flows"):                  # the arena changed
            m.scan_flowbits()
        with raises(ESTATE, "no packet metadata"):
            m.build_flows()
        m.set_meta(meta_of_flows(flow))
        m.build_flows()
        check(m, base, flow, SESSION, 2)
        # every refusal leaves the ops before it in force
        for rows, n_bits, text in [([(0, 0, 2, 0)], 0, "n_bits is 0, outside 1..32"), ([(0, 0, 2, 0)], 33, "n_bits is 33, outside 1..32"),
                                   ([(N_RULES, 0, 2, 0)], 1, f"op 0 names rule {N_RULES} of {N_RULES}"), ([(0, 2, 0, 0)], 2, "op 0 names bit 2 of 2"),
                                   ([(0, 0, 6, 0)], 1, "op 0: 6 is none of KMPGPU_FB_"), ([(0, 0, 2, 1)], 1, "op 0: the reserved field is 1, not 0"),
                                   ([(1, 0, 0, 0), (1, 0, 1, 0)], 1, "op 1: rule 1 tests bit 0 both set and clear"),
                                   ([(0, 0, 0, 0), (0, 1, 2, 0), (1, 1, 0, 0), (1, 0, 4, 0)], 2, "the flow bits 0 -> 1 -> 0 form a cycle"),
                                   ([(0, 2, 0, 0), (0, 0, 2, 0), (1, 0, 1, 0), (1, 1, 3, 0), (2, 1, 0, 0), (2, 2, 2, 0)], 3,
                                    "the flow bits 0 -> 1 -> 2 -> 0 form a cycle")]:
            with raises(EINVAL, text):
                _set_raw(m, rows, n_bits)
            check(m, base, flow, SESSION, 2, raw=False)
        with raises(EINVAL, "ops is NULL"):
            _lib.gpu_check(m._g.kmpgpu_set_flowbits(m._ctx, None, 1, 1), "kmpgpu_set_flowbits")
        # a self-loop is accepted; clearing; new rules drop the ops, and so do new patterns
        m.set_flowbits([(2, "isset", 0), (2, "unset", 0), (5, "set", 0)])
        check(m, base, flow, [(2, "isset", 0), (2, "unset", 0), (5, "set", 0)], 1)
        m.set_flowbits([])
        with raises(ESTATE, "no flow bits"):
            m.scan_flowbits()
        m.set_flowbits(SESSION)
        m.set_rules(RULES)
        with raises(ESTATE, "no flow bits"):
            m.scan_flowbits()
        m.set_flowbits(SESSION)
        m.set_patterns(PATS)
        with raises(ESTATE, "no rules set"):
            m.scan_flowbits()
        # the Python layer's own checks
        for bad in ([(0, "flip", 0)], [(0, "set")], [(0, "noalert", 1)], [(0,)]):
            with pytest.raises(ValueError):
                m.set_flowbits(bad)
    finally:
        m.close()


def test_the_other_calls_are_what_they_were(gm):
    """scan_rules, scan_flows and load_seams give the same bits before and after the flow-bit calls"""
    n = TILE + 1
    masks = masks_of(n, 13)
    flow = np.arange(n) % 64
    sm = GpuMatcher(0)
    try:
        sm.set_patterns(PATS)

        def snapshot():
            rules = gm.scan_rules(hits=True)
            folded = gm.scan_flows("rules", "flow", hits=True)
            n_seams = sm.load_seams(gm, 8)
            return (rules["hits"].tobytes(), rules["rule_pkt_counts"].tobytes(), rules["any"].tobytes(), rules["timing"].launches,
                    folded["hits"].tobytes(), folded["flow_counts"].tobytes(), folded["timing"].launches, n_seams, sm.seams().tobytes(),
                    [a.tobytes() for a in sm.arena_download()], sm.last_timing().launches)
        setup(gm, masks)
        gm.set_meta(meta_of_flows(flow, seed=2))
        gm.build_flows()
        before = snapshot()
        gm.set_flowbits(SESSION)
        gm.scan_flowbits(hits=True, state=True)
        assert snapshot() == before
        gm.scan_flowbits()
        gm.set_flowbits([])
        assert snapshot() == before
    finally:
        sm.close()


# ------------------------------------------------------------------------------------------------
# 4. the command line
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"])])
def test_cli_on_a_tcp_capture(tmp_path, prog, extra):
    """tests/golden/data/tcp.pcap: one conversation of 13 segments, four of them a GET and one the answer"""
    arena = HostArena.from_pcap(os.path.join(DATA, "tcp.pcap"), "tcp", with_meta=True)
    payloads = [bytes(arena.bytes[int(o):int(o) + int(ln)]) for o, ln in zip(arena.off, arena.len)]
    pats = [b"GET", b"204", b"Host:"]
    hits = MM.hits(MM.starts(payloads, pats), len(pats))
    assert hits[0].sum() > 1 and hits[1].any()
    rules = [([0, 2], []), ([1], []), ([0], [])]
    base = MM.rule_rows(hits, rules)
    strings, rules_f, fb_f, alerts = (tmp_path / name for name in ("strings.txt", "rules.txt", "flowbits.txt", "alerts.csv"))
    strings.write_bytes(b"\n".join(pats) + b"\n")
    rules_f.write_text("0 2\n1\n0\n")
    fb_f.write_text("# the first request of a connection, and the answer only behind a request\n0 isnotset:req set:req\n\n1 isset:req\n2 noalert toggle:odd\n")
    ops = [(0, "isnotset", 0), (0, "set", 0), (1, "isset", 0), (2, "noalert"), (2, "toggle", 1)]
    plain = run_cli(prog, "tcp.pcap", str(strings), extra, mode="tcp")
    assert plain.returncode == 0, plain.stderr
    for directed in (False, True):
        env = {"KMPGPU_RULES_FILE": str(rules_f), "KMPGPU_ALERTS_FILE": str(alerts), "KMPGPU_FLOWBITS_FILE": str(fb_f)}
        if directed:
            env["KMPGPU_FLOWS_DIRECTED"] = "1"
        r = run_cli(prog, "tcp.pcap", str(strings), extra, env_extra=env, mode="tcp")
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == strip_elapsed(plain.stdout)
        fo = FM.flow_of(arena.meta, directed)
        assert (len(set(fo.tolist())) == 2) == directed
        want = FB.run(base, fo, ops, 2)["alert"]
        assert want[0].sum() == 1 and want[1].any() != directed and not want[2].any()
        assert alerts.read_text() == "".join(f"{k},{r}\n" for k, r in sorted((int(k), int(r)) for r, k in np.argwhere(want)))
