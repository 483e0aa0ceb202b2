"""The definition of kmpgpu_http_locate / kmpgpu_load_fields (include/kmpgpu.h) in plain Python with index arithmetic: what the GPU
tests compare the library with, byte for byte.  No device needed.

Every term is "the smallest index with a local property": e the first '\\n' (or L), e' the start line's end without its '\\r', s1 / s2
the first two ' ' in front of e', bl the first '\\n' that a blank line follows.  tests/test_http_model.py holds this against a second
formulation through `re`."""
import numpy as np

from decode_model import packed_image, words

NONE, REQUEST, RESPONSE = 0, 1, 2
HAS_LF, HAS_BLANK, HAS_TOKEN = 1, 2, 4
FIELDS = {"method": 1, "raw_uri": 2, "status": 3, "headers": 4, "body": 5}
STEP = 1024            # bytes of a payload the locate takes at a time (kmpgpu_http_stats.bytes_scanned is defined in these)

SPAN_DTYPE = np.dtype([("kind", np.uint8), ("flags", np.uint8), ("method_len", np.uint16), ("tok_off", np.uint32), ("tok_len", np.uint32),
                       ("hdr_off", np.uint32), ("hdr_len", np.uint32), ("body_off", np.uint32), ("body_len", np.uint32),
                       ("reserved", np.uint32)])
assert SPAN_DTYPE.itemsize == 32


def first(p: bytes, byte: int, lo: int, hi: int):
    """the smallest i in [lo, hi) with p[i] == byte, or None"""
    for i in range(lo, hi):
        if p[i] == byte:
            return i
    return None


def locate(p: bytes) -> dict:
    """Every term of the definition for one payload.  Absent fields are None, present ones (offset, length)."""
    L = len(p)
    e = first(p, 0x0A, 0, L)
    has_lf = e is not None
    if e is None:
        e = L
    e1 = e - 1 if e >= 1 and p[e - 1] == 0x0D else e
    s1 = first(p, 0x20, 0, e1)
    s2 = None
    if s1 is not None:
        s2 = first(p, 0x20, s1 + 1, e1)
        if s2 is None:
            s2 = e1
    if e1 >= 5 and p[0:5] == b"HTTP/":
        kind = RESPONSE
    elif s1 is not None and 1 <= s1 <= 15 and all(0x41 <= c <= 0x5A for c in p[0:s1]) and s1 + 1 < e1:
        kind = REQUEST
    else:
        kind = NONE
    out = {"kind": kind, "e": e, "e1": e1, "s1": s1, "s2": s2, "bl": None, "method": None, "raw_uri": None, "status": None, "headers": None,
           "body": None}
    # the blank line (looked for whatever the kind: bytes_scanned of a NONE payload does not need it, its fields are absent)
    bl, b0 = None, None
    if has_lf:
        for i in range(e, L):
            if p[i] != 0x0A:
                continue
            if i + 1 < L and p[i + 1] == 0x0A:
                bl, b0 = i, i + 2
                break
            if i + 2 < L and p[i + 1] == 0x0D and p[i + 2] == 0x0A:
                bl, b0 = i, i + 3
                break
    out["bl"] = bl
    if kind == NONE:
        return out
    if kind == REQUEST:
        out["method"] = (0, s1)
        out["raw_uri"] = (s1 + 1, s2 - s1 - 1)
    elif s1 is not None and s1 + 1 < e1:
        out["status"] = (s1 + 1, s2 - s1 - 1)
    if has_lf:
        h1 = bl + 1 if bl is not None else L
        out["headers"] = (e + 1, h1 - (e + 1))
    if bl is not None:
        out["body"] = (b0, L - b0)
    return out


def candidate(p: bytes) -> bool:
    """what the first 16-byte unit alone does not rule out (the kernel reads on only in these payloads)"""
    if len(p) >= 5 and p[0:5] == b"HTTP/":
        return True
    u = p[:16]
    s = u.find(b" ")
    return s >= 1 and all(0x41 <= c <= 0x5A for c in u[:s])


def bytes_scanned(p: bytes, t: dict) -> int:
    """kmpgpu_http_stats.bytes_scanned of one payload (kmpgpu.h)"""
    L = len(p)
    if not candidate(p):
        return min(L, 16)
    if t["kind"] == NONE:
        stop = t["e"]                                  # left at the step that ends the start line
    else:
        stop = t["bl"] if t["bl"] is not None else L - 1
    stop = min(stop, L - 1)
    return min(L, STEP * (stop // STEP + 1))


def span(p: bytes) -> tuple:
    """the kmpgpu_http_span record of one payload, as a tuple in SPAN_DTYPE's order"""
    t = locate(p)
    if t["kind"] == NONE:
        return (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    tok = t["raw_uri"] if t["kind"] == REQUEST else t["status"]
    flags = (HAS_LF if t["headers"] is not None else 0) | (HAS_BLANK if t["body"] is not None else 0) | (HAS_TOKEN if tok is not None else 0)
    z = (0, 0)
    return (t["kind"], flags, t["method"][1] if t["method"] else 0) + (tok or z) + (t["headers"] or z) + (t["body"] or z) + (0,)


def spans(payloads) -> np.ndarray:
    return np.array([span(t) for t in payloads], dtype=SPAN_DTYPE)


def locate_stats(payloads) -> dict:
    ts = [locate(t) for t in payloads]
    return {"n_requests": sum(t["kind"] == REQUEST for t in ts), "n_responses": sum(t["kind"] == RESPONSE for t in ts),
            "n_blank": sum(t["kind"] != NONE and t["bl"] is not None for t in ts),
            "bytes_scanned": sum(bytes_scanned(p, t) for p, t in zip(payloads, ts))}


def field(p: bytes, name: str):
    """the bytes of one field of a payload, or None where it is absent"""
    r = locate(p)[name]
    return None if r is None else p[r[0]:r[0] + r[1]]


def load_fields(payloads, name: str, only_present: bool = False) -> dict:
    """What dst holds after kmpgpu_load_fields over these payloads, and what the call hands out (the image dict of
    decode_model.load_decoded, `present` in the place of `changed`)."""
    got = [field(t, name) for t in payloads]
    present = np.array([g is not None for g in got], dtype=bool)
    index = np.flatnonzero(present).astype(np.int64) if only_present else np.arange(len(payloads), dtype=np.int64)
    out = [got[int(k)] or b"" for k in index]
    arena, off, ln = packed_image(out)
    return {"payloads": out, "arena": arena, "off": off, "len": ln, "present": present, "words": words(present), "index": index,
            "stats": {"n_payloads": len(out), "n_present": int(present.sum()), "bytes_in": sum(len(payloads[int(k)]) for k in index),
                      "bytes_out": sum(len(t) for t in out)}}
