"""The host model of flow streams by TCP sequence number: numpy, bytes and Python loops, no GPU, nothing of the library.  Written from the
definition of include/kmpgpu.h ("Flow streams by TCP sequence number") on top of tests/stream_model.py (members, slots, arena):
    a stream is TCP iff meta[first member in capture order].proto == 6; every other stream is tests/stream_model.py's
    rel(k) = int32(seq[k] - seq[k0]), off(k) = rel(k) - min rel, order = ascending (off, k)
    byte x of the sequence space = payload_k[x - off(k)] of the FIRST k in that order that covers x
    stream = the covered x in ascending order, holes closed, cut to depth
The bytes are placed in a per-stream dict {sequence offset: (byte, payload, offset in payload)} filled in (off, k) order with setdefault:
there is no running maximum here, which is how the kernels (and kept_by_maximum below) do it.
"""
import numpy as np

import stream_model as TM

SEG_DTYPE = np.dtype([("skip", "<u4"), ("take", "<u4"), ("seq_off", "<u4"), ("reserved", "<u4")])
ORDER_DTYPE = np.dtype([("seq_base", "<u4"), ("n_gaps", "<u4"), ("gap_bytes", "<u8"), ("dup_bytes", "<u8"), ("tcp", "<u4"), ("reserved", "<u4")])


def rel(a, b):
    """(int32_t)(uint32_t)(a - b)"""
    d = (int(a) - int(b)) & 0xFFFFFFFF
    return d - (1 << 32) if d >= 1 << 31 else d


def stream_cells(pay, ks, seq):
    """one TCP stream: (members in (off, k) order, {k: off}, {x: (byte, k, offset in k)})"""
    rels = {k: rel(seq[k], seq[ks[0]]) for k in ks}
    low = min(rels.values())
    off = {k: rels[k] - low for k in ks}
    order = sorted(ks, key=lambda k: (off[k], k))
    cells = {}
    for k in order:
        for j, byte in enumerate(pay[k]):
            cells.setdefault(off[k] + j, (byte, k, j))
    return order, off, cells


def build(pay, meta, seq, depth, directed=False, fo=None):
    """(streams' bytes, STREAM_DTYPE[n_streams], STREAM_POS_DTYPE[n], SEG_DTYPE[n], ORDER_DTYPE[n_streams], origin) where origin[s] is
    the list of (payload, offset in payload) of every byte of stream s before the cut"""
    assert 1 <= depth <= TM.DEPTH_MAX
    ms = TM.members(meta, directed, fo)
    n = len(pay)
    recs = np.zeros(len(ms), dtype=TM.STREAM_DTYPE)
    pos = np.zeros(n, dtype=TM.STREAM_POS_DTYPE)
    segs = np.zeros(n, dtype=SEG_DTYPE)
    orders = np.zeros(len(ms), dtype=ORDER_DTYPE)
    streams, origin = [], []
    for s, (f, d, ks) in enumerate(ms):
        r = recs[s]
        r["first_packet"], r["last_packet"], r["n_packets"], r["flow"], r["dir"] = ks[0], ks[-1], len(ks), f, d
        if int(meta[ks[0]]["proto"]) != 6:
            at, src = 0, []
            for k in ks:
                pos[k]["stream"], pos[k]["pos"] = s, at
                segs[k]["take"] = len(pay[k])
                src += [(k, j) for j in range(len(pay[k]))]
                at += len(pay[k])
            data = b"".join(bytes(pay[k]) for k in ks)
        else:
            order, off, cells = stream_cells(pay, ks, seq)
            xs = sorted(cells)
            data = bytes(cells[x][0] for x in xs)
            src = [cells[x][1:] for x in xs]
            rank = {x: i for i, x in enumerate(xs)}
            # what a member contributes: the cells it owns.  They are a suffix of it; its position is the rank of the first one, and the
            # position of a member that owns nothing is the number of cells in front of its place in the order
            before = 0
            seen = -1                                           # the highest x placed so far
            gaps = gap_bytes = 0
            for i, k in enumerate(order):
                own = [j for j in range(len(pay[k])) if cells[off[k] + j][1] == k]
                assert own == list(range(len(pay[k]) - len(own), len(pay[k])))
                segs[k]["skip"], segs[k]["take"], segs[k]["seq_off"] = len(pay[k]) - len(own), len(own), off[k]
                pos[k]["stream"], pos[k]["pos"] = s, rank[off[k] + own[0]] if own else before
                before += len(own)
                if i and off[k] > seen + 1:
                    gaps, gap_bytes = gaps + 1, gap_bytes + off[k] - (seen + 1)
                seen = max(seen, off[k] + len(pay[k]) - 1)
            # (the gaps are defined through M(k); a zero-length member behind every byte opens one too, so max(xs) does not bound them)
            assert before == len(xs) and gap_bytes == seen + 1 - len(xs)
            o = orders[s]
            o["tcp"], o["n_gaps"], o["gap_bytes"] = 1, gaps, gap_bytes
            o["dup_bytes"] = sum(len(pay[k]) for k in ks) - len(xs)
            o["seq_base"] = (int(seq[ks[0]]) + min(rel(seq[k], seq[ks[0]]) for k in ks)) & 0xFFFFFFFF
        r["bytes"], r["len"] = len(data), min(len(data), depth)
        streams.append(data[:depth])
        origin.append(src)
    return streams, recs, pos, segs, orders, origin


def build_np(lens, meta, seq, depth, directed=False):
    """(recs, pos, segs, orders) of build without the Python loops and without the bytes, for hundreds of thousands of payloads: the
    members sorted by (stream, off, k) with one lexsort, then the running maximum of off + L inside every stream, the kernels' formulation
    (kept_by_maximum below).  Every stream's ends are moved behind those of the stream before it (stream << 33: an end is below 2^33), so
    one maximum.accumulate serves all streams.  tests/test_streams_seq_high_model.py holds it to build."""
    assert 1 <= depth <= TM.DEPTH_MAX
    lens, seq = np.asarray(lens, dtype=np.int64), np.asarray(seq).astype(np.uint32).astype(np.int64)
    recs, pos = TM.records_np(meta, lens, depth, directed)              # first, last, n_packets, flow, dir; pos["stream"]
    n, S = len(lens), len(recs)
    segs, orders = np.zeros(n, dtype=SEG_DTYPE), np.zeros(S, dtype=ORDER_DTYPE)
    if n == 0:
        return recs, pos, segs, orders
    st = pos["stream"].astype(np.int64)
    first = recs["first_packet"].astype(np.int64)
    tcp = np.asarray(meta["proto"])[first] == 6
    r = (seq - seq[first][st]) & 0xFFFFFFFF
    r = np.where(tcp[st], np.where(r >= 1 << 31, r - (1 << 32), r), 0)
    low = np.full(S, 1 << 40, dtype=np.int64)
    np.minimum.at(low, st, r)
    off = r - low[st]
    k = np.lexsort((np.arange(n), off, st))
    ks, ko, kL = st[k], off[k], lens[k]
    head = np.ones(n, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    hp = np.flatnonzero(head)
    ep = np.concatenate([hp[1:], [n]])
    incl = np.maximum.accumulate(ks << 33 | np.where(tcp[ks], ko + kL, 0))         # (a stream that is not TCP covers nothing)
    M = np.where(head, 0, np.concatenate([[0], incl[:-1]]) & ((1 << 33) - 1))       # exclusive, 0 at every stream's first member
    skip = np.clip(M - ko, 0, kL)
    take = kL - skip
    gap = ~head & (ko > M) & tcp[ks]
    excl = np.cumsum(take) - take
    kept = np.add.reduceat(take, hp)
    segs["skip"][k], segs["take"][k], segs["seq_off"][k] = skip, take, ko
    pos["pos"][k] = excl - excl[hp][ks]
    recs["bytes"], recs["len"] = kept, np.minimum(kept, depth)
    orders["tcp"] = tcp
    orders["n_gaps"] = np.add.reduceat(gap.astype(np.int64), hp)
    orders["gap_bytes"] = np.where(tcp, (incl[ep - 1] & ((1 << 33) - 1)) - kept, 0)
    orders["dup_bytes"] = np.add.reduceat(kL, hp) - kept
    orders["seq_base"] = np.where(tcp, (seq[first] + low) & 0xFFFFFFFF, 0)
    return recs, pos, segs, orders


def kept_by_maximum(lens, offs):
    """[(skip, take)] of members given in (off, k) order by the running maximum, the kernels' formulation: skip = min(L, max(0, M - off))"""
    out, M = [], 0
    for L, o in zip(lens, offs):
        skip = min(L, max(0, M - o))
        out.append((skip, L - skip))
        M = max(M, o + L)
    return out
