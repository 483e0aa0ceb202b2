"""The host model of the byte tests (kmpgpu_set_bytetests, include/kmpgpu.h): plain Python over the in-window matches of
tests/match_model.py, written from the definition and from nothing of the library.

A test is a dict as GpuMatcher.set_bytetests takes it: nbytes, op, value, offset, and optionally mask, anchor (its presence makes the
test relative) and flags (LITTLE).  `bt` builds one.

    E_k            the payload's text end: its first 0x00, or its length under `whole`
    field(k, pos)  bytes pos .. pos + nbytes - 1 of payload k as an integer, defined only for 0 <= pos and pos + nbytes <= E_k
    absolute       field(k, offset) is defined and ((field & mask) op value)
    relative       the same for field(k, s + len(anchor) + offset) of SOME in-window match s of the anchor
The field's bytes are the payload's own, also where the anchor is a nocase pattern.
"""
import numpy as np

import match_model as MM

RELATIVE, LITTLE = 1, 2
EQ, NE, LT, GT, LE, GE = range(6)
U32 = 0xFFFFFFFF


def bt(nbytes, op, value, offset, mask=U32, anchor=None, little=False):
    t = dict(nbytes=nbytes, op=op, value=value, offset=offset, mask=mask, flags=LITTLE if little else 0)
    if anchor is not None:
        t["anchor"] = anchor
    return t


def isdataat(n):
    """Snort's isdataat:N: a byte exists at offset n"""
    return bt(1, GE, 0, n)


def field(text, end, pos, nbytes, little):
    """None where the field is not defined"""
    if pos < 0 or pos + nbytes > end:
        return None
    v = 0
    for i in range(nbytes):
        b = text[pos + i]
        v = v | b << (8 * i) if little else v << 8 | b
    return v


def holds(f, t):
    if f is None:
        return False
    x, v = f & t.get("mask", U32), t["value"]
    return {EQ: x == v, NE: x != v, LT: x < v, GT: x > v, LE: x <= v, GE: x >= v}[t["op"]]


def bytetest_rows(payloads, pats, tests, windows=None, nocase=None, whole=False, st=None):
    """bool[n_bt, n_pkts].  st: MM.starts(payloads, pats, windows, nocase, whole) where the caller has it already"""
    if st is None and any("anchor" in t for t in tests):
        st = MM.starts(payloads, pats, windows, nocase, whole)
    rows = np.zeros((len(tests), len(payloads)), dtype=bool)
    for k, text in enumerate(payloads):
        end = MM.text_end(text, whole)
        for q, t in enumerate(tests):
            little = bool(t.get("flags", 0) & LITTLE)
            if "anchor" not in t:
                rows[q, k] = holds(field(text, end, t["offset"], t["nbytes"], little), t)
                continue
            a = t["anchor"]
            for s in st[k][a]:
                if holds(field(text, end, s + len(pats[a]) + t["offset"], t["nbytes"], little), t):
                    rows[q, k] = True
                    break
    return rows
