"""The host model of flows: numpy and a Python dict keyed by the tuple, no GPU, nothing of the library.  Written from the definitions of
include/kmpgpu.h ("Flows"): with M = meta[k], e_src = src_ip << 16 | src_port and e_dst = dst_ip << 16 | dst_port,
    key(k) = (proto, min(e_src, e_dst), max(e_src, e_dst))      by default
    key(k) = (proto, e_src, e_dst)                              directed
two payloads are one flow iff their keys are equal, flows are numbered in the order of their first payload.

flow_of / records are that definition, record by record.  flow_of_np / records_np give the same arrays from numpy's sort of the key
columns, for the captures of hundreds of thousands of payloads that tests/test_gpu_rows_scale.py builds.
"""
import numpy as np

import match_model as MM
from header_model import META_DTYPE

FLOW_DTYPE = np.dtype([("first_packet", "<u8"), ("last_packet", "<u8"), ("n_packets", "<u8"), ("payload_bytes", "<u8"), ("first", META_DTYPE)])


def key(m, directed=False):
    es = int(m["src_ip"]) << 16 | int(m["src_port"])
    ed = int(m["dst_ip"]) << 16 | int(m["dst_port"])
    if not directed and ed < es:
        es, ed = ed, es
    return int(m["proto"]), es, ed


def flow_of(meta, directed=False):
    """uint32[n_pkts]: every payload's flow"""
    ids = {}
    out = np.zeros(len(meta), dtype=np.uint32)
    for k, m in enumerate(meta):
        out[k] = ids.setdefault(key(m, directed), len(ids))
    return out


def records(meta, lens, directed=False):
    """FLOW_DTYPE[n_flows]"""
    fo = flow_of(meta, directed)
    n_flows = int(fo.max()) + 1 if len(fo) else 0
    recs = np.zeros(n_flows, dtype=FLOW_DTYPE)
    seen = np.zeros(n_flows, dtype=bool)
    for k, f in enumerate(fo):
        r = recs[f]
        if not seen[f]:
            seen[f] = True
            r["first_packet"] = k
            r["first"] = meta[k]
        r["last_packet"] = k
        r["n_packets"] += 1
        r["payload_bytes"] += int(lens[k])
    return recs


def key_columns(meta, directed=False):
    """uint64[n, 3]: the key's columns (proto, e_src, e_dst), the endpoints swapped into ascending order unless directed"""
    es = meta["src_ip"].astype(np.uint64) << np.uint64(16) | meta["src_port"].astype(np.uint64)
    ed = meta["dst_ip"].astype(np.uint64) << np.uint64(16) | meta["dst_port"].astype(np.uint64)
    if not directed:
        es, ed = np.minimum(es, ed), np.maximum(es, ed)
    return np.stack([meta["proto"].astype(np.uint64), es, ed], axis=1)


def _first_and_flow(meta, directed):
    """(first payload of every flow, ascending; uint32[n_pkts] flow of every payload): the distinct rows of the key columns, renumbered by
    the index at which each appears first"""
    if len(meta) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32)
    # what np.unique(cols, axis=0, return_index=True, return_inverse=True) gives, by three stable sorts of one column each instead of one
    # sort of whole rows (seconds instead of half a minute for millions of payloads): inside a key the payloads stay in capture order,
    # so the first one of a group is the key's first payload
    cols = key_columns(meta, directed)
    by_key = np.lexsort((cols[:, 2], cols[:, 1], cols[:, 0]))
    s = cols[by_key]
    new = np.ones(len(s), dtype=bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    first = by_key[new]
    inv = np.empty(len(s), dtype=np.int64)
    inv[by_key] = np.cumsum(new) - 1
    order = np.argsort(first, kind="stable")          # the distinct keys in the order of their first payload
    rank = np.empty(len(first), dtype=np.uint32)
    rank[order] = np.arange(len(first), dtype=np.uint32)
    return first[order].astype(np.int64), rank[np.asarray(inv).reshape(-1)]


def flow_of_np(meta, directed=False):
    """flow_of without the Python loop: for hundreds of thousands of payloads.  tests/test_flow_model.py holds it to flow_of."""
    return _first_and_flow(meta, directed)[1]


def records_np(meta, lens, directed=False):
    """records without the Python loop, byte for byte the same"""
    return flows_np(meta, lens, directed)[1]


def flows_np(meta, lens, directed=False):
    """(flow_of_np, records_np) from one sort of the keys"""
    first, fo = _first_and_flow(meta, directed)
    return fo, _records_np(meta, lens, first, fo)


def _records_np(meta, lens, first, fo):
    recs = np.zeros(len(first), dtype=FLOW_DTYPE)
    if len(first) == 0:
        return recs
    k = np.arange(len(fo), dtype=np.uint64)
    recs["first_packet"] = first
    recs["first"] = meta[first]
    recs["n_packets"] = np.bincount(fo, minlength=len(first))
    bytes_, last = np.zeros(len(first), dtype=np.uint64), np.zeros(len(first), dtype=np.uint64)
    np.add.at(bytes_, fo, np.asarray(lens).astype(np.uint64))
    np.maximum.at(last, fo, k)
    recs["payload_bytes"], recs["last_packet"] = bytes_, last
    return recs


def fold(rows, fo, n_flows=None):
    """bool[n_rows, n_pkts] -> bool[n_rows, n_flows]: flow f is in a row where one of its payloads is"""
    n_flows = (int(fo.max()) + 1 if len(fo) else 0) if n_flows is None else n_flows
    out = np.zeros((rows.shape[0], n_flows), dtype=bool)
    for r in range(rows.shape[0]):
        out[r, fo[rows[r]]] = True
    return out


def flow_rules(term_rows, fo, rules, n_flows=None):
    """bool[n_rules, n_flows] of the (all_of, none_of) rules under KMPGPU_FLOW_SCOPE_FLOW: every term row folded, then the rule per flow"""
    return MM.rule_rows(fold(term_rows, fo, n_flows), rules)


def expand(flow_bits, fo):
    """bool[n_flows] -> bool[n_pkts]"""
    return np.asarray(flow_bits, dtype=bool)[fo] if len(fo) else np.zeros(0, dtype=bool)


def dotted(ip):
    return ".".join(str(int(ip) >> s & 255) for s in (24, 16, 8, 0))


def flows_file(recs):
    """what KMPGPU_FLOWS_FILE holds: flow,proto,src,sport,dst,dport,first_payload,last_payload,payloads,bytes"""
    return "".join(f"{f},{int(r['first']['proto'])},{dotted(r['first']['src_ip'])},{int(r['first']['src_port'])},{dotted(r['first']['dst_ip'])},"
                   f"{int(r['first']['dst_port'])},{int(r['first_packet'])},{int(r['last_packet'])},{int(r['n_packets'])},{int(r['payload_bytes'])}\n"
                   for f, r in enumerate(recs))


def flow_alerts_file(rule_rows):
    """what KMPGPU_FLOW_ALERTS_FILE holds: one flow,rule line per set bit of bool[n_rules, n_flows], sorted by flow, then rule"""
    return "".join(f"{f},{r}\n" for f, r in sorted((int(f), int(r)) for r, f in np.argwhere(rule_rows)))
