"""The host model of the header predicates: numpy and bytes only, no GPU, nothing of the library.

Two halves, both written from the byte rules of include/kmpgpu.h:
  frame -> (accepted, payload offset, payload length, metadata) for the udp and the tcp extractor (`extract`), and with it a pure-Python
  reader of classic pcap files (`pcap_frames`) -- what the fixtures' accepted payloads are counted with;
  (metadata, payload lengths, predicates) -> predicate rows (`header_rows`).
"""
import struct

import numpy as np

META_DTYPE = np.dtype([("src_ip", "<u4"), ("dst_ip", "<u4"), ("src_port", "<u2"), ("dst_port", "<u2"), ("proto", "u1"), ("reserved", "u1", (3,))])
ANY_PROTO, BIDIR = 1, 2
U32_MAX = 0xFFFFFFFF


def extract(p, cl, mode):
    """None for a frame the extractor of `mode` ("udp" / "tcp") rejects, else (payload offset, payload length, meta tuple
    (src_ip, dst_ip, src_port, dst_port, proto)).  p: the frame's bytes, cl: its captured length (only p[:cl] is looked at)."""
    if mode == "udp":
        if cl < 34:
            return None
        ihl = (p[14] & 0x0F) << 2
        rest = cl - 14
        if rest < ihl or p[23] != 17 or rest - ihl < 8:
            return None
        off, ln = 14 + ihl + 8, rest - ihl - 8
    else:
        if cl < 15:
            return None
        ihl = (p[14] & 0x0F) << 2
        t = 14 + ihl
        if ihl < 20 or cl < t + 13:
            return None
        size_tcp = (p[t + 12] >> 4) << 2
        if size_tcp < 20 or cl < t + size_tcp:
            return None
        off, ln = t + size_tcp, cl - (t + size_tcp)
    t = 14 + ((p[14] & 0x0F) << 2)
    assert t + 4 <= cl and 34 <= cl                    # every byte the metadata reads lies inside the captured bytes
    src = p[26] << 24 | p[27] << 16 | p[28] << 8 | p[29]
    dst = p[30] << 24 | p[31] << 16 | p[32] << 8 | p[33]
    return off, ln, (src, dst, p[t] << 8 | p[t + 1], p[t + 2] << 8 | p[t + 3], p[23])


def pcap_frames(path):
    """[(caplen, frame bytes)] of a classic pcap file, either byte order; a truncated last record ends the list"""
    with open(path, "rb") as f:
        b = f.read()
    magic = struct.unpack("<I", b[:4])[0]
    e = "<" if magic in (0xA1B2C3D4, 0xA1B23C4D) else ">"
    assert struct.unpack(e + "I", b[:4])[0] in (0xA1B2C3D4, 0xA1B23C4D), path
    out, pos = [], 24
    while pos + 16 <= len(b):
        cl = struct.unpack(e + "I", b[pos + 8:pos + 12])[0]
        if pos + 16 + cl > len(b):
            break
        out.append((cl, b[pos + 16:pos + 16 + cl]))
        pos += 16 + cl
    return out


def meta_array(metas):
    a = np.zeros(len(metas), dtype=META_DTYPE)
    for r, (s, d, sp, dp, pr) in zip(a, metas):
        r["src_ip"], r["dst_ip"], r["src_port"], r["dst_port"], r["proto"] = s, d, sp, dp, pr
    return a


def capture(frames, mode):
    """(payloads [bytes], META_DTYPE[n]) of the frames the extractor of `mode` accepts, in order.  frames: [(caplen, bytes)]"""
    pay, metas = [], []
    for cl, p in frames:
        r = extract(p, cl, mode)
        if r is not None:
            pay.append(bytes(p[r[0]:r[0] + r[1]]))
            metas.append(r[2])
    return pay, meta_array(metas)


def header(proto=None, src=(0, 0), dst=(0, 0), sport=(0, 0xFFFF), dport=(0, 0xFFFF), length=(0, U32_MAX), bidir=False):
    """one predicate as the dict GpuMatcher.set_headers takes; proto None: any"""
    h = dict(src_ip=src[0], src_mask=src[1], dst_ip=dst[0], dst_mask=dst[1], sport_lo=sport[0], sport_hi=sport[1], dport_lo=dport[0],
             dport_hi=dport[1], len_lo=length[0], len_hi=length[1], flags=(BIDIR if bidir else 0) | (ANY_PROTO if proto is None else 0))
    if proto is not None:
        h["proto"] = proto
    return h


def _dir(h, s, d, sp, dp):
    """one direction of a predicate over arrays of addresses and ports (int64)"""
    return (((s & h["src_mask"]) == (h["src_ip"] & h["src_mask"])) & ((d & h["dst_mask"]) == (h["dst_ip"] & h["dst_mask"]))
            & (h["sport_lo"] <= sp) & (sp <= h["sport_hi"]) & (h["dport_lo"] <= dp) & (dp <= h["dport_hi"]))


def header_rows(meta, lens, headers):
    """bool[n_hdr, n_pkts]: the definition of include/kmpgpu.h, predicate by predicate over all payloads.  headers: dicts as `header`
    makes them (a missing proto with ANY_PROTO set is never read)"""
    s, d, sp, dp, pr = (meta[f].astype(np.int64) for f in ("src_ip", "dst_ip", "src_port", "dst_port", "proto"))
    ln = np.asarray(lens).astype(np.int64)
    rows = np.zeros((len(headers), len(ln)), dtype=bool)
    for q, h in enumerate(headers):
        fl = h.get("flags", 0)
        ok = (ln >= h["len_lo"]) & (ln <= h["len_hi"])
        if not fl & ANY_PROTO:
            ok &= pr == h.get("proto", 0)
        way = _dir(h, s, d, sp, dp)
        if fl & BIDIR:
            way |= _dir(h, d, s, dp, sp)
        rows[q] = ok & way
    return rows


def make_frame(mode, payload, src, dst, sport, dport, proto=None, ihl=5, tcp_words=5):
    """an Ethernet / IP / transport frame around payload the way the extractors read one: IHL in the low nibble of byte 14, the
    protocol in byte 23, addresses in bytes 26..33, the ports at the transport header's start; in tcp mode the data offset in
    the high nibble of transport byte 12.  Option bytes of a longer IP / TCP header are 0xEE."""
    proto = (17 if mode == "udp" else 6) if proto is None else proto
    ip = bytearray(b"\xEE" * (ihl * 4))
    ip[0] = 0x40 | ihl
    ip[9] = proto
    ip[12:16] = struct.pack(">I", src)
    ip[16:20] = struct.pack(">I", dst)
    if mode == "udp":
        tr = struct.pack(">HHHH", sport, dport, 8 + len(payload), 0)
    else:
        tr = bytearray(b"\xEE" * (tcp_words * 4))
        tr[0:4] = struct.pack(">HH", sport, dport)
        tr[12] = tcp_words << 4
        tr = bytes(tr)
    return bytes(b"\x02" * 12 + b"\x08\x00" + bytes(ip) + tr + payload)


def write_pcap(path, frames):
    """a classic little-endian pcap of [(caplen, bytes)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1))
        for i, (cl, p) in enumerate(frames):
            f.write(struct.pack("<IIII", i, 0, cl, len(p)) + bytes(p[:cl]))
