"""The host model of flow streams: numpy, bytes and Python loops, no GPU, nothing of the library.  Written from the definitions of
include/kmpgpu.h ("Flow streams") on top of tests/flow_model.py and tests/seam_model.py (flow_of, direction):
    a stream is one distinct (flow_of, dir); streams are numbered in ascending order of flow << 1 | dir
    its members are the payloads of that flow and direction in capture order
    stream s = payload_k0[0:L] ++ payload_k1[0:L] ++ ..., cut to its first `depth` bytes
and the records, the per-payload map, the arena kmpgpu_load_streams leaves (slots of max(16, round_up(len, 16)) bytes back to back from 0,
0x00 behind every stream's end) and the metadata that goes with it.
"""
import numpy as np

import flow_model as FM
import seam_model as SM

STREAM_DTYPE = np.dtype([("first_packet", "<u8"), ("last_packet", "<u8"), ("n_packets", "<u8"), ("bytes", "<u8"), ("flow", "<u4"),
                         ("dir", "<u4"), ("len", "<u4"), ("reserved", "<u4")])
STREAM_POS_DTYPE = np.dtype([("stream", "<u4"), ("reserved", "<u4"), ("pos", "<u8")])
DEPTH_MAX = 1 << 30


def members(meta, directed=False, fo=None):
    """[(flow, dir, [k0, k1, ...])] in stream order: the members of every stream in capture order"""
    fo = FM.flow_of(meta, directed) if fo is None else fo
    dr = SM.direction(meta, fo)
    chains = {}
    for k in range(len(meta)):
        chains.setdefault((int(fo[k]), int(dr[k])), []).append(k)
    return [(f, d, chains[(f, d)]) for f, d in sorted(chains)]


def records(meta, lens, depth, directed=False, fo=None):
    """(STREAM_DTYPE[n_streams], STREAM_POS_DTYPE[n_pkts])"""
    assert 1 <= depth <= DEPTH_MAX
    ms = members(meta, directed, fo)
    recs = np.zeros(len(ms), dtype=STREAM_DTYPE)
    pos = np.zeros(len(meta), dtype=STREAM_POS_DTYPE)
    for s, (f, d, ks) in enumerate(ms):
        at = 0
        for k in ks:
            pos[k]["stream"], pos[k]["pos"] = s, at
            at += int(lens[k])
        r = recs[s]
        r["first_packet"], r["last_packet"], r["n_packets"], r["bytes"] = ks[0], ks[-1], len(ks), at
        r["flow"], r["dir"], r["len"] = f, d, min(at, depth)
    return recs, pos


def records_np(meta, lens, depth, directed=False):
    """records without the Python loops, for hundreds of thousands of payloads: a stable sort by (flow, dir) keeps capture order inside
    every stream.  tests/test_stream_model.py holds it to records."""
    fo, frecs = FM.flows_np(meta, lens, directed)
    n = len(fo)
    pos = np.zeros(n, dtype=STREAM_POS_DTYPE)
    if n == 0:
        return np.zeros(0, dtype=STREAM_DTYPE), pos
    f1 = frecs["first"][fo]
    dr = ~((meta["src_ip"] == f1["src_ip"]) & (meta["src_port"] == f1["src_port"]) & (meta["dst_ip"] == f1["dst_ip"])
           & (meta["dst_port"] == f1["dst_port"]))
    key = fo.astype(np.uint64) << np.uint64(1) | dr.astype(np.uint64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(n, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    hp = np.flatnonzero(head)
    ep = np.concatenate([hp[1:], [n]])
    sn = np.cumsum(head) - 1
    L = np.asarray(lens, dtype=np.int64)[order]
    excl = np.cumsum(L) - L
    total = np.concatenate([excl, [int(L.sum())]])
    pos["stream"][order] = sn
    pos["pos"][order] = excl - excl[hp][sn]
    recs = np.zeros(len(hp), dtype=STREAM_DTYPE)
    recs["first_packet"], recs["last_packet"], recs["n_packets"] = order[hp], order[ep - 1], ep - hp
    recs["bytes"] = total[ep] - total[hp]
    recs["flow"], recs["dir"] = ks[hp] >> np.uint64(1), ks[hp] & np.uint64(1)
    recs["len"] = np.minimum(recs["bytes"], depth)
    return recs, pos


def payloads(pay, meta, depth, directed=False, fo=None):
    """the streams' bytes"""
    return [b"".join(bytes(pay[k]) for k in ks)[:depth] for _, _, ks in members(meta, directed, fo)]


def slot(n):
    return max(16, (n + 15) // 16 * 16)


def arena(streams):
    """(bytes, off uint64[n], len uint32[n]) of the packed arena: every slot whole, 0x00 behind the stream's end; what
    kmpgpu_arena_download returns without the 64 bytes the library keeps behind the last slot"""
    return SM.arena(streams)


def locate(pos, lens, stream, offset):
    """(payload, offset in it) of byte `offset` of stream `stream`, by walking the stream's members"""
    at = 0
    for k in [k for k in range(len(pos)) if int(pos[k]["stream"]) == stream]:
        assert int(pos[k]["pos"]) == at
        if offset < at + int(lens[k]):
            return k, offset - at
        at += int(lens[k])
    raise ValueError("offset behind the stream's end")
