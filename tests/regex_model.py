"""The host model of the regex rows (kmpgpu_set_regexes, include/kmpgpu.h): Python's re on bytes, and the gate.  Written from the
definition and from nothing of the library.

An expression is what GpuMatcher.set_regexes takes: ``bytes``, or ``(bytes, dict(nocase=, dotall=, gate=))``; `rx` builds one.

    E_k           the payload's text end: its first 0x00, or its length under `whole`
    rx_hit[q][k]  re.compile(expr_q, with a trailing $ rewritten to \\Z; re.I for nocase, re.S for dotall).search(payload_k[:E_k]) is not None,
                  and, where the expression has a gate, the gate pattern's row of scan_packets holds payload k
$ is the text end alone: Python's \\Z, not Python's $, which also matches in front of a final newline.
"""
import re

import numpy as np

import match_model as MM

NOCASE, DOTALL, GATED = 1, 2, 4


def rx(expr, nocase=False, dotall=False, gate=None):
    opt = {}
    if nocase:
        opt["nocase"] = True
    if dotall:
        opt["dotall"] = True
    if gate is not None:
        opt["gate"] = gate
    return (expr, opt) if opt else expr


def parts(e):
    """(expr, nocase, dotall, gate or None) of either form"""
    expr, opt = (e, {}) if isinstance(e, (bytes, bytearray)) else e
    return bytes(expr), bool(opt.get("nocase")), bool(opt.get("dotall")), opt.get("gate")


def ends_with_dollar(expr):
    """a trailing $ that no backslash escapes"""
    if not expr.endswith(b"$"):
        return False
    body = expr[:-1]
    return (len(body) - len(body.rstrip(b"\\"))) % 2 == 0


def compiled(expr, nocase=False, dotall=False):
    if ends_with_dollar(expr):
        expr = expr[:-1] + b"\\Z"
    return re.compile(expr, (re.I if nocase else 0) | (re.S if dotall else 0))


def search(expr, text, nocase=False, dotall=False, whole=False):
    """the verdict on one text, without a gate"""
    return compiled(expr, nocase, dotall).search(bytes(text[:MM.text_end(text, whole)])) is not None


def regex_rows(payloads, exprs, whole=False, pattern_hits=None):
    """bool[n_rx, n_pkts].  pattern_hits: bool[n_pat, n_pkts], the rows of scan_packets (MM.hits(MM.starts(...))), read for the gated
    expressions only"""
    rows = np.zeros((len(exprs), len(payloads)), dtype=bool)
    texts = [bytes(t[:MM.text_end(t, whole)]) for t in payloads]
    for q, e in enumerate(exprs):
        expr, nocase, dotall, gate = parts(e)
        c = compiled(expr, nocase, dotall)
        rows[q] = [c.search(t) is not None for t in texts]
        if gate is not None:
            rows[q] &= np.asarray(pattern_hits[gate], dtype=bool)
    return rows
