"""The definition of kmpgpu_dns_locate / kmpgpu_load_dns (include/kmpgpu.h) in plain Python: what the GPU tests compare the library
with, record by record and byte by byte.  No device needed.

The walk is the definition's, step by step: i_0 = 12, c = m[i_t], 0 ends the name, 1..63 is a label, anything else makes the payload
NONE.  tests/test_dns_model.py holds this against hand-written verdicts, dnspython and the golden table of the fixtures."""
import struct

import numpy as np

from decode_model import packed_image, words

NONE, QUERY, RESPONSE = 0, 1, 2
NAME_WIRE_MAX = 255

SPAN_DTYPE = np.dtype([("kind", np.uint8), ("n_labels", np.uint8), ("flags", np.uint16), ("id", np.uint16), ("qtype", np.uint16),
                       ("qclass", np.uint16), ("qdcount", np.uint16), ("ancount", np.uint16), ("nscount", np.uint16), ("arcount", np.uint16),
                       ("reserved", np.uint16), ("name_off", np.uint32), ("name_len", np.uint32), ("q_end", np.uint32)])
assert SPAN_DTYPE.itemsize == 32


def locate(p: bytes, tcp_prefix: bool = False):
    """Every term of the definition for one payload: None for NONE, otherwise a dict with the record's fields, i_end and the name."""
    b = 2 if tcp_prefix else 0
    m = p[b:]
    M = len(p) - b
    if M < 17:
        return None
    ident, flags, qd, an, ns, ar = struct.unpack(">6H", m[:12])
    if qd < 1:
        return None
    i, seps, n_labels = 12, [], 0
    while True:
        if not i < M:
            return None
        c = m[i]
        if c == 0:
            break
        if c >= 64 or i + 1 + c > M:
            return None
        if i > 12:
            seps.append(i)
        n_labels += 1
        i += 1 + c
    i_end = i
    if i_end + 1 - 12 > NAME_WIRE_MAX or i_end + 5 > M:
        return None
    name = bytearray(m[13:i_end])
    for s in seps:
        name[s - 13] = 0x2E
    qtype, qclass = struct.unpack(">2H", m[i_end + 1:i_end + 5])
    return {"kind": RESPONSE if flags & 0x8000 else QUERY, "n_labels": n_labels, "flags": flags, "id": ident, "qtype": qtype, "qclass": qclass,
            "qdcount": qd, "ancount": an, "nscount": ns, "arcount": ar, "name_off": b + 13, "name_len": max(0, i_end - 13),
            "q_end": b + i_end + 5, "i_end": i_end, "name": bytes(name)}


def qname(p: bytes, tcp_prefix: bool = False):
    """the dotted name of a payload's first question, or None where the payload is NONE"""
    t = locate(p, tcp_prefix)
    return None if t is None else t["name"]


def span(p: bytes, tcp_prefix: bool = False) -> tuple:
    """the kmpgpu_dns_span record of one payload, as a tuple in SPAN_DTYPE's order"""
    t = locate(p, tcp_prefix)
    if t is None:
        return (0,) * 14
    return (t["kind"], t["n_labels"], t["flags"], t["id"], t["qtype"], t["qclass"], t["qdcount"], t["ancount"], t["nscount"], t["arcount"], 0,
            t["name_off"], t["name_len"], t["q_end"])


def spans(payloads, tcp_prefix: bool = False) -> np.ndarray:
    return np.array([span(t, tcp_prefix) for t in payloads], dtype=SPAN_DTYPE)


def locate_stats(payloads, tcp_prefix: bool = False) -> dict:
    ts = [t for t in (locate(p, tcp_prefix) for p in payloads) if t is not None]
    return {"n_queries": sum(t["kind"] == QUERY for t in ts), "n_responses": sum(t["kind"] == RESPONSE for t in ts),
            "n_root": sum(t["i_end"] == 12 for t in ts), "name_bytes": sum(t["name_len"] for t in ts)}


def load_dns(payloads, only_present: bool = False, tcp_prefix: bool = False) -> dict:
    """What dst holds after kmpgpu_load_dns over these payloads, and what the call hands out (the image dict of
    http_model.load_fields)."""
    got = [qname(t, tcp_prefix) for t in payloads]
    present = np.array([g is not None for g in got], dtype=bool)
    index = np.flatnonzero(present).astype(np.int64) if only_present else np.arange(len(payloads), dtype=np.int64)
    out = [got[int(k)] or b"" for k in index]
    arena, off, ln = packed_image(out)
    return {"payloads": out, "arena": arena, "off": off, "len": ln, "present": present, "words": words(present), "index": index,
            "stats": {"n_payloads": len(out), "n_present": int(present.sum()), "bytes_in": sum(len(payloads[int(k)]) for k in index),
                      "bytes_out": sum(len(t) for t in out)}}


def message(labels, qtype: int = 1, qclass: int = 1, ident: int = 0x1234, flags: int = 0x0100, qd: int = 1, an: int = 0, ns: int = 0, ar: int = 0,
            tail: bytes = b"", tcp_prefix: bool = False) -> bytes:
    """A DNS message with one question whose name has these labels (bytes each, taken as they are, any length), and `tail` behind it."""
    wire = b"".join(bytes([len(x) & 0xFF]) + x for x in labels) + b"\x00"
    msg = struct.pack(">6H", ident, flags, qd, an, ns, ar) + wire + struct.pack(">2H", qtype, qclass) + tail
    return (struct.pack(">H", len(msg) & 0xFFFF) if tcp_prefix else b"") + msg
