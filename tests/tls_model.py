"""The definition of kmpgpu_tls_locate / kmpgpu_load_tls (include/kmpgpu.h) in plain Python: what the GPU tests compare the library
with, record by record and byte by byte.  No device needed.

The walk is the definition's, clause by clause, in its order.  tests/test_tls_model.py holds this against hand-written verdicts, the
golden ClientHellos OpenSSL produced (tests/golden/tls_hellos.json) and every prefix of them."""
import struct

import numpy as np

from decode_model import packed_image, words

NONE, CLIENT_HELLO = 0, 1
HAS_SNI, HAS_ALPN, TRUNCATED, ALPN_SKIPPED = 1, 2, 4, 8
EXT_MAX, ALPN_MAX = 255, 256

SPAN_DTYPE = np.dtype([("kind", np.uint8), ("flags", np.uint8), ("n_ext", np.uint8), ("sid_len", np.uint8), ("record_version", np.uint16),
                       ("client_version", np.uint16), ("n_suites", np.uint16), ("n_alpn", np.uint16), ("hs_len", np.uint32),
                       ("sni_off", np.uint32), ("sni_len", np.uint32), ("alpn_off", np.uint32), ("alpn_len", np.uint32)])
assert SPAN_DTYPE.itemsize == 32
SPAN_FIELDS = SPAN_DTYPE.names


def be16(p, i):
    return p[i] << 8 | p[i + 1]


def locate(p: bytes):
    """Every term of the definition for one payload: None for NONE, otherwise a dict with the record's fields and "sni" / "alpn" (bytes,
    or None where the field is absent)."""
    L = len(p)
    # the fixed header
    if not (L >= 11 and p[0] == 22 and p[1] == 3 and p[2] <= 4 and p[5] == 1 and p[9] == 3):
        return None
    rec, hs = be16(p, 3), p[6] << 16 | p[7] << 8 | p[8]
    if not rec >= hs + 4:
        return None
    t = {"kind": CLIENT_HELLO, "flags": 0, "n_ext": 0, "sid_len": 0, "record_version": be16(p, 1), "client_version": be16(p, 9), "n_suites": 0,
         "n_alpn": 0, "hs_len": hs, "sni_off": 0, "sni_len": 0, "alpn_off": 0, "alpn_len": 0, "sni": None, "alpn": None}
    # the fixed part
    H = 9 + hs
    E = min(L, H)
    if not 43 < E:
        return None
    sid = p[43]
    if not sid <= 32:
        return None
    t["sid_len"] = sid
    c = 44 + sid
    if not c + 2 <= E:
        return None
    cs = be16(p, c)
    if cs % 2 or cs < 2:
        return None
    t["n_suites"] = cs // 2
    c += 2 + cs
    if not c < E:
        return None
    cm = p[c]
    if not cm >= 1:
        return None
    c += 1 + cm
    if c == H:
        return t
    if not c + 2 <= E:
        return None
    X = c + 2 + be16(p, c)
    if X != H:
        return None
    c += 2
    Xe = min(X, E)
    if Xe < X:
        t["flags"] |= TRUNCATED
    # the extension walk
    sni_seen = alpn_seen = False
    while c + 4 <= Xe:
        ty, n, b = be16(p, c), be16(p, c + 2), c + 4
        if b + n > X:
            return None
        if b + n > Xe:
            break
        t["n_ext"] += 1
        if t["n_ext"] > EXT_MAX:
            return None
        if ty == 0 and not sni_seen:
            sni_seen = True
            if not n >= 5:
                return None
            ll = be16(p, b)
            if not ll + 2 <= n or p[b + 2] != 0:
                return None
            nl = be16(p, b + 3)
            if not 3 + nl <= ll:
                return None
            t["flags"] |= HAS_SNI
            t["sni_off"], t["sni_len"], t["sni"] = b + 5, nl, bytes(p[b + 5:b + 5 + nl])
        elif ty == 16 and not alpn_seen:
            alpn_seen = True
            if not n >= 4:
                return None
            ll = be16(p, b)
            if ll + 2 != n or ll < 2:
                return None
            if ll > ALPN_MAX:
                t["flags"] |= ALPN_SKIPPED
            else:
                q, end, seps, names = b + 2, b + 2 + ll, [], 0
                while q < end:
                    l = p[q]
                    if l < 1 or q + 1 + l > end:
                        return None
                    if q > b + 2:
                        seps.append(q)
                    names += 1
                    q += 1 + l
                field = bytearray(p[b + 3:b + 2 + ll])
                for s in seps:
                    field[s - (b + 3)] = 0x2C
                t["flags"] |= HAS_ALPN
                t["alpn_off"], t["alpn_len"], t["n_alpn"], t["alpn"] = b + 3, ll - 1, names, bytes(field)
        c = b + n
    if not t["flags"] & TRUNCATED and c != X:
        return None
    return t


def field_of(p: bytes, field: str):
    """"sni" or "alpn" of a payload; None where the payload is NONE or has no such field"""
    t = locate(p)
    return None if t is None else t[field]


def span(p: bytes) -> tuple:
    """the kmpgpu_tls_span record of one payload, as a tuple in SPAN_DTYPE's order"""
    t = locate(p)
    return (0,) * len(SPAN_FIELDS) if t is None else tuple(t[f] for f in SPAN_FIELDS)


def spans(payloads) -> np.ndarray:
    return np.array([span(t) for t in payloads], dtype=SPAN_DTYPE)


def locate_stats(payloads) -> dict:
    ts = [t for t in (locate(p) for p in payloads) if t is not None]
    return {"n_hellos": len(ts), "n_sni": sum(bool(t["flags"] & HAS_SNI) for t in ts), "n_alpn": sum(bool(t["flags"] & HAS_ALPN) for t in ts),
            "n_truncated": sum(bool(t["flags"] & TRUNCATED) for t in ts)}


def load_tls(payloads, field: str = "sni", only_present: bool = False) -> dict:
    """What dst holds after kmpgpu_load_tls over these payloads, and what the call hands out (the image dict of
    http_model.load_fields)."""
    got = [field_of(t, field) for t in payloads]
    present = np.array([g is not None for g in got], dtype=bool)
    index = np.flatnonzero(present).astype(np.int64) if only_present else np.arange(len(payloads), dtype=np.int64)
    out = [got[int(k)] or b"" for k in index]
    arena, off, ln = packed_image(out)
    return {"payloads": out, "arena": arena, "off": off, "len": ln, "present": present, "words": words(present), "index": index,
            "stats": {"n_payloads": len(out), "n_present": int(present.sum()), "bytes_in": sum(len(payloads[int(k)]) for k in index),
                      "bytes_out": sum(len(t) for t in out)}}


# ---- a small builder: a ClientHello from its parts, every length field overridable, so that each clause can be missed by one ----

def ext(ty: int, body: bytes, n=None) -> bytes:
    return struct.pack(">HH", ty, len(body) if n is None else n) + body


def sni_ext(name: bytes, ll=None, nl=None, name_type: int = 0, tail: bytes = b"", n=None) -> bytes:
    """the server_name extension: one host_name entry, `tail` behind it inside the list (a second entry, say)"""
    entry = bytes([name_type]) + struct.pack(">H", len(name) if nl is None else nl) + name + tail
    return ext(0, struct.pack(">H", len(entry) if ll is None else ll) + entry, n)


def alpn_ext(names, ll=None, n=None) -> bytes:
    """the ALPN extension; names: bytes each (its length byte is len & 0xFF), or an int for a bare length byte"""
    body = b"".join(bytes([x]) if isinstance(x, int) else bytes([len(x) & 0xFF]) + x for x in names)
    return ext(16, struct.pack(">H", len(body) if ll is None else ll) + body, n)


def hello(exts=(), sid: int = 32, suites: int = 3, cm: bytes = b"\x00", rec_ver: int = 0x0301, ver: int = 0x0303, hs=None, rec=None, xlen=None,
          hs_type: int = 1, rec_type: int = 22, sid_byte=None, cs=None, no_ext_block: bool = False, tail: bytes = b"") -> bytes:
    """A record that holds one ClientHello with these extensions (already encoded, see ext); `tail` stands behind the record."""
    xs = b"".join(exts)
    body = struct.pack(">H", ver) + bytes(range(32)) + bytes([sid if sid_byte is None else sid_byte]) + bytes(0xA0 + (i & 15) for i in range(sid))
    body += struct.pack(">H", 2 * suites if cs is None else cs) + b"\x13\x01" * suites + bytes([len(cm)]) + cm
    if not no_ext_block:
        body += struct.pack(">H", len(xs) if xlen is None else xlen) + xs
    hsl = len(body) if hs is None else hs
    msg = bytes([hs_type]) + struct.pack(">I", hsl)[1:] + body
    return bytes([rec_type]) + struct.pack(">H", rec_ver) + struct.pack(">H", len(msg) if rec is None else rec) + msg + tail
