"""Flow bits (kmpgpu_set_flowbits / kmpgpu_scan_flowbits; include/kmpgpu.h) as a plain sequential loop over a dict of flows, written from
the definition alone: for every flow, payload after payload in capture order, B = the state before the payload; a rule fires where its
base bit is set and all its tests hold on B; the fired rules' actions, rules in ascending index and a rule's actions in the order given,
make the state the next payload of the flow sees; a rule with "noalert" fires and acts but does not alert.

An op is (rule, "set" | "unset" | "toggle" | "isset" | "isnotset", bit) or (rule, "noalert"), as GpuMatcher.set_flowbits takes them.
"""
import numpy as np

TESTS, ACTIONS = ("isset", "isnotset"), ("set", "unset", "toggle")


def run(base, flow_of, ops, n_bits):
    """base: bool[n_rules, n] (what scan_rules gives), flow_of: int[n].  Returns a dict: ``alert`` and ``fired`` bool[n_rules, n],
    ``state`` bool[n_bits, n] (bit X before payload k), ``flow_state`` uint32[n_flows] (after the flow's last payload; flows are
    numbered 0 .. max(flow_of))."""
    base = np.asarray(base, dtype=bool)
    n_rules, n = base.shape
    flow_of = [int(f) for f in flow_of]
    assert len(flow_of) == n
    by_rule = {r: [] for r in range(n_rules)}
    noalert = set()
    for op in ops:
        if op[1] == "noalert":
            noalert.add(int(op[0]))
        else:
            assert op[1] in TESTS + ACTIONS and 0 <= int(op[2]) < n_bits
            by_rule[int(op[0])].append((op[1], int(op[2])))
    fired = np.zeros((n_rules, n), dtype=bool)
    before = np.zeros(n, dtype=np.uint64)              # B of every payload
    rules_of = [[] for _ in range(n)]                  # the rules whose base bit payload k has, ascending
    for r, k in np.argwhere(base).tolist():
        rules_of[k].append(r)
    states = {}                                        # flow -> S
    for k in range(n):
        B = states.get(flow_of[k], 0)
        S = B
        before[k] = B
        for r in rules_of[k]:
            if not all(bool(B >> X & 1) == (what == "isset") for what, X in by_rule[r] if what in TESTS):
                continue
            fired[r, k] = True
            for what, X in by_rule[r]:
                if what == "set":
                    S |= 1 << X
                elif what == "unset":
                    S &= ~(1 << X)
                elif what == "toggle":
                    S ^= 1 << X
        states[flow_of[k]] = S
    state = np.array([(before >> np.uint64(X)) & np.uint64(1) for X in range(n_bits)], dtype=bool).reshape(n_bits, n)
    alert = fired.copy()
    for r in noalert:
        alert[r] = False
    flow_state = np.zeros(max(flow_of) + 1 if n else 0, dtype=np.uint32)
    for f, S in states.items():
        flow_state[f] = S
    return {"alert": alert, "fired": fired, "state": state, "flow_state": flow_state}


def levels(ops, n_bits):
    """level[X] = the longest path into bit X in the graph with an edge Y -> X where a rule tests Y and acts on X != Y; None with a cycle."""
    tests, acts = {}, {}
    for op in ops:
        if op[1] in TESTS:
            tests.setdefault(int(op[0]), set()).add(int(op[2]))
        elif op[1] in ACTIONS:
            acts.setdefault(int(op[0]), set()).add(int(op[2]))
    edges = {(y, x) for r in tests for y in tests[r] for x in acts.get(r, ()) if x != y}
    level = [0] * n_bits
    for _ in range(n_bits + 1):
        moved = False
        for y, x in edges:
            if level[x] < level[y] + 1:
                level[x], moved = level[y] + 1, True
        if not moved:
            return level
    return None
