"""The host model of content chains (kmpgpu_set_chains): what every exact comparison of tests/test_gpu_chains.py rests on.  It sits on
tests/match_model.py's `starts` and nothing else; tests/test_chain_model.py holds it to an enumeration of all tuples.

A chain is (p0, (p1, dmin, dmax), (p2, dmin, dmax), ...): it holds in a payload where matches s_0 .. s_{n-1} of p_0 .. p_{n-1} exist with
dmin_j <= s_j - (s_{j-1} + len(p_{j-1})) <= dmax_j for every link j; a bound of None: that side is open.  chain_rows goes stage by
stage from that definition: the starts of content j that some tuple of the contents before it reaches.
"""
import bisect
import itertools

import numpy as np

from match_model import I32_MAX, I32_MIN


def links(chain):
    """[(pattern, dmin, dmax)] with the first content's open bounds written out"""
    return [(chain[0], None, None)] + [tuple(l) for l in chain[1:]]


def chain_holds(row, pats, chain):
    """row: the in-window starts per pattern of one payload (match_model.starts()[k])"""
    ls = links(chain)
    reach = list(row[ls[0][0]])                       # the starts of content 0 (ascending, as `starts` gives them)
    for (prev, _, _), (p, dmin, dmax) in zip(ls, ls[1:]):
        lo = I32_MIN if dmin is None else dmin
        hi = I32_MAX if dmax is None else dmax
        m = len(pats[prev])
        # s stays iff some reached start t of the content before has lo <= s - (t + m) <= hi, i.e. s - m - hi <= t <= s - m - lo:
        # the first t at or above the lower end decides
        nxt = []
        for s in row[p]:
            i = bisect.bisect_left(reach, s - m - hi)
            if i < len(reach) and reach[i] <= s - m - lo:
                nxt.append(s)
        reach = nxt
        if not reach:
            return False
    return bool(reach)


def chain_holds_all_tuples(row, pats, chain):
    """the definition itself: some tuple out of the product of the contents' starts"""
    ls = links(chain)
    for tup in itertools.product(*[row[p] for p, _, _ in ls]):
        if all((I32_MIN if lo is None else lo) <= tup[j] - (tup[j - 1] + len(pats[ls[j - 1][0]])) <= (I32_MAX if hi is None else hi)
               for j, (_, lo, hi) in enumerate(ls) if j):
            return True
    return False


def chain_rows(st, pats, chains):
    """bool[n_chains, n_pkts]"""
    rows = np.zeros((len(chains), len(st)), dtype=bool)
    for k, row in enumerate(st):
        memo = {}
        for c, chain in enumerate(chains):
            if all(row[p] for p, _, _ in links(chain)):
                if chain not in memo:
                    memo[chain] = chain_holds(row, pats, chain)
                rows[c, k] = memo[chain]
    return rows


def pairwise_relations(chain):
    """the relations (a, b, dmin, dmax) of a chain's links, each on its own: what a rule of relations can ask for"""
    ls = links(chain)
    return [(a[0], b[0], b[1], b[2]) for a, b in zip(ls, ls[1:])]


def flat_chains(chains):
    """(chain_off uint32[n + 1], [(pattern, dmin, dmax)] with the INT32 ends written out) as kmpgpu_set_chains takes them"""
    off = np.zeros(len(chains) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(ch) for ch in chains])
    flat = [(p, I32_MIN if lo is None else lo, I32_MAX if hi is None else hi) for ch in chains for p, lo, hi in links(ch)]
    return off, flat
