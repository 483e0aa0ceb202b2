"""The host model of flow seams: numpy, bytes and Python loops, no GPU, nothing of the library.  Written from the definitions of
include/kmpgpu.h ("Flow seams") on top of tests/flow_model.py and tests/match_model.py:
    dir(k)  = 0 where payload k's (e_src, e_dst) equal those of its flow's first payload, else 1 (always 0 for directed flows)
    pred(k) = the largest j < k with flow_of[j] == flow_of[k] and dir(j) == dir(k)
    one seam per payload with a predecessor, numbered in ascending order of `next`:
        payload_prev[L_prev - tail_len : L_prev] ++ payload_next[0 : head_len],  tail_len = min(reach, L_prev), head_len = min(reach, L_next)
and the arena kmpgpu_load_seams leaves (slots of max(16, round_up(len, 16)) bytes back to back from 0, 0x00 behind every seam's end), the
metadata and seam_flow that go with it, and the term rows of kmpgpu_scan_flows_seams.
"""
import numpy as np

import flow_model as FM
import match_model as MM

SEAM_DTYPE = np.dtype([("prev", "<u8"), ("next", "<u8"), ("tail_len", "<u4"), ("head_len", "<u4")])
NONE = -1


def endpoints(m):
    return (int(m["src_ip"]) << 16 | int(m["src_port"]), int(m["dst_ip"]) << 16 | int(m["dst_port"]))


def direction(meta, fo):
    """uint8[n_pkts]: dir(k).  The flow's first payload is the lowest k of the flow."""
    first = {}
    out = np.zeros(len(meta), dtype=np.uint8)
    for k, m in enumerate(meta):
        e = endpoints(m)
        out[k] = 0 if first.setdefault(int(fo[k]), e) == e else 1
    return out


def pred(fo, dr):
    """int64[n_pkts]: pred(k), NONE without one"""
    last = {}
    out = np.full(len(fo), NONE, dtype=np.int64)
    for k in range(len(fo)):
        key = (int(fo[k]), int(dr[k]))
        out[k] = last.get(key, NONE)
        last[key] = k
    return out


def records(meta, lens, reach, directed=False, fo=None):
    """SEAM_DTYPE[n_seams], in ascending order of `next`"""
    fo = FM.flow_of(meta, directed) if fo is None else fo
    pr = pred(fo, direction(meta, fo))
    nxt = np.flatnonzero(pr != NONE)
    recs = np.zeros(len(nxt), dtype=SEAM_DTYPE)
    recs["prev"], recs["next"] = pr[nxt], nxt
    lens = np.asarray(lens, dtype=np.int64)
    recs["tail_len"] = np.minimum(reach, lens[pr[nxt]])
    recs["head_len"] = np.minimum(reach, lens[nxt])
    return recs


def records_np(meta, lens, reach, directed=False):
    """records without the Python loops, for hundreds of thousands of payloads: a stable sort by (flow, dir) keeps capture order inside
    every chain, so a payload's predecessor is its neighbour in the sorted order.  tests/test_seam_model.py holds it to records."""
    fo, frecs = FM.flows_np(meta, lens, directed)
    n = len(fo)
    if n == 0:
        return np.zeros(0, dtype=SEAM_DTYPE)
    f1 = frecs["first"][fo]
    dr = ~((meta["src_ip"] == f1["src_ip"]) & (meta["src_port"] == f1["src_port"]) & (meta["dst_ip"] == f1["dst_ip"])
           & (meta["dst_port"] == f1["dst_port"]))
    key = fo.astype(np.uint64) << np.uint64(1) | dr.astype(np.uint64)
    order = np.argsort(key, kind="stable")
    same = np.zeros(n, dtype=bool)
    same[1:] = key[order[1:]] == key[order[:-1]]
    pr = np.full(n, NONE, dtype=np.int64)
    pr[order[same]] = order[np.flatnonzero(same) - 1]
    nxt = np.flatnonzero(pr != NONE)
    recs = np.zeros(len(nxt), dtype=SEAM_DTYPE)
    lens = np.asarray(lens, dtype=np.int64)
    recs["prev"], recs["next"] = pr[nxt], nxt
    recs["tail_len"], recs["head_len"] = np.minimum(reach, lens[pr[nxt]]), np.minimum(reach, lens[nxt])
    return recs


def payloads(pay, recs):
    """the seams' bytes"""
    out = []
    for r in recs:
        p, q = pay[int(r["prev"])], pay[int(r["next"])]
        out.append(bytes(p[len(p) - int(r["tail_len"]):]) + bytes(q[: int(r["head_len"])]))
    return out


def slot(n):
    return max(16, (n + 15) // 16 * 16)


def arena(seams):
    """(bytes, off uint64[n], len uint32[n]) of the packed arena: every slot whole, 0x00 behind the seam's end; what kmpgpu_arena_download
    returns without the 64 bytes the library keeps behind the last slot"""
    ln = np.array([len(s) for s in seams], dtype=np.uint32)
    size = np.array([slot(len(s)) for s in seams], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64) if len(seams) else np.zeros(0, dtype=np.uint64)
    body = b"".join(s + b"\0" * (slot(len(s)) - len(s)) for s in seams)
    return np.frombuffer(body, dtype=np.uint8), off, ln


def combined_terms(src_terms, seam_hits, fo, seam_flow, n_flows):
    """bool[n_terms, n_flows]: the folded term rows of kmpgpu_scan_flows_seams.  src_terms: bool[n_terms, n_pkts], the rows the rule terms
    index in src (patterns first); seam_hits: bool[n_pat, n_seams], the hit matrix of the seams under the seam context's own options.
    Only the pattern rows take the seams' bits."""
    out = FM.fold(src_terms, fo, n_flows)
    n_pat = seam_hits.shape[0]
    if seam_hits.shape[1]:
        out[:n_pat] |= FM.fold(seam_hits, seam_flow, n_flows)
    return out


def flow_rules(src_terms, seam_hits, fo, seam_flow, rules, n_flows):
    """bool[n_rules, n_flows] of kmpgpu_scan_flows_seams"""
    return MM.rule_rows(combined_terms(src_terms, seam_hits, fo, seam_flow, n_flows), rules)
