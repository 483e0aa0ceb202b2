"""tests/http_model.py, the definition of kmpgpu_http_locate / kmpgpu_load_fields in index arithmetic: hand-written verdicts for every
clause of the definition (include/kmpgpu.h), and agreement with a second, independent formulation through `re` on bytes.  No device
needed."""
import re

import numpy as np
import pytest

import http_model as HM

N, Q, R = HM.NONE, HM.REQUEST, HM.RESPONSE


def fields(p):
    t = HM.locate(p)
    return t["kind"], tuple(None if t[f] is None else p[t[f][0]:t[f][0] + t[f][1]] for f in ("method", "raw_uri", "status", "headers", "body"))


# (payload, kind, method, raw_uri, status, headers, body); None: absent
VERDICTS = [
    # a plain request, both line ends
    (b"GET /a HTTP/1.1\r\nHost: x\r\n\r\nbody", Q, b"GET", b"/a", None, b"Host: x\r\n", b"body"),
    (b"GET /a HTTP/1.1\nHost: x\n\nbody", Q, b"GET", b"/a", None, b"Host: x\n", b"body"),
    # start line end: no '\n' at all -> e = L, no headers, no body; a trailing '\r' is still taken off
    (b"GET /a", Q, b"GET", b"/a", None, None, None),
    (b"GET /a\r", Q, b"GET", b"/a", None, None, None),
    (b"GET /a b\r", Q, b"GET", b"/a", None, None, None),
    # s2: the second ' ', or e'
    (b"GET /a b c\n", Q, b"GET", b"/a", None, b"", None),
    (b"GET  x\n", Q, b"GET", b"", None, b"", None),                      # RAW_URI may be empty
    # s1 + 1 < e': something has to follow the ' '
    (b"GET \n", N, None, None, None, None, None),
    (b"GET \r\n", N, None, None, None, None, None),
    (b"GET x\n", Q, b"GET", b"x", None, b"", None),
    (b"GET \rx\n", Q, b"GET", b"\rx", None, b"", None),                   # a '\r' that is not in front of the '\n' is a byte like any other
    # method: 1 .. 15 upper-case letters
    (b"A b", Q, b"A", b"b", None, None, None),
    (b" GET /", N, None, None, None, None, None),                         # s1 == 0
    (b"ABCDEFGHIJKLMNO /x", Q, b"ABCDEFGHIJKLMNO", b"/x", None, None, None),
    (b"ABCDEFGHIJKLMNOP /x", N, None, None, None, None, None),            # 16 letters
    (b"get /x", N, None, None, None, None, None),
    (b"GeT /x", N, None, None, None, None, None),
    (b"G3T /x", N, None, None, None, None, None),
    (b"GET\n/x y", N, None, None, None, None, None),                      # the ' ' lies behind e'
    (b"", N, None, None, None, None, None),
    (b"G", N, None, None, None, None, None),
    # responses
    (b"HTTP/1.1 200 OK\r\nServer: y\r\n\r\n<html>", R, None, None, b"200", b"Server: y\r\n", b"<html>"),
    (b"HTTP/", R, None, None, None, None, None),                          # "HTTP/" alone
    (b"HTTP", N, None, None, None, None, None),
    (b"HTTP\n/", N, None, None, None, None, None),                        # e' < 5
    (b"HTTP/1.1 ", R, None, None, None, None, None),                      # STATUS needs s1 + 1 < e'
    (b"HTTP/1.1 \r\n", R, None, None, None, b"", None),
    (b"HTTP/1.1  x", R, None, None, b"", None, None),                     # ... and may be empty
    (b"HTTP/1.1 404", R, None, None, b"404", None, None),
    (b"HTTP/ 1 2\n\n", R, None, None, b"1", b"", b""),
    # headers: present iff e < L; cut by the segment where there is no blank line
    (b"GET /a HTTP/1.1\n", Q, b"GET", b"/a", None, b"", None),
    (b"GET /a HTTP/1.1\r\nHost: x\r\nUser-Agent", Q, b"GET", b"/a", None, b"Host: x\r\nUser-Agent", None),
    (b"GET /a HTTP/1.1\r\nHost: x\r\n", Q, b"GET", b"/a", None, b"Host: x\r\n", None),
    # bl == e: empty headers, still present
    (b"GET /a\n\nB", Q, b"GET", b"/a", None, b"", b"B"),
    (b"GET /a\r\n\r\nB", Q, b"GET", b"/a", None, b"", b"B"),
    # the blank line's forms need their bytes inside the payload; the body may be empty
    (b"GET /a\nH: 1\n\n", Q, b"GET", b"/a", None, b"H: 1\n", b""),
    (b"GET /a\nH: 1\n\r\n", Q, b"GET", b"/a", None, b"H: 1\n", b""),
    (b"GET /a\nH: 1\n\r", Q, b"GET", b"/a", None, b"H: 1\n\r", None),
    (b"GET /a\nH: 1\n", Q, b"GET", b"/a", None, b"H: 1\n", None),
    (b"GET /a\nH: 1\n\rx\n\n!", Q, b"GET", b"/a", None, b"H: 1\n\rx\n", b"!"),       # "\n\r" without its '\n' is no blank line
    (b"GET /a\nH\r\n\nB", Q, b"GET", b"/a", None, b"H\r\n", b"B"),                   # mixed: "\r\n" then "\n"
    (b"GET /a\nH\n\r\n\r\nB", Q, b"GET", b"/a", None, b"H\n", b"\r\nB"),             # the first one counts
    # 0x00 is a byte like any other
    (b"GET /a\nH:\x00\n\nB\x00", Q, b"GET", b"/a", None, b"H:\x00\n", b"B\x00"),
    # NONE: every field is absent, whatever follows
    (b"hello\r\n\r\nworld", N, None, None, None, None, None),
]


@pytest.mark.parametrize("case", VERDICTS, ids=[repr(c[0])[:40] for c in VERDICTS])
def test_verdicts(case):
    p, kind, *want = case
    assert fields(p) == (kind, tuple(want))


def test_spans_and_image():
    pay = [b"GET /a HTTP/1.1\r\nHost: x\r\n\r\nbody", b"dns", b"HTTP/1.1 200 OK\n\n", b"", b"POST  HTTP/1.1\n"]
    s = HM.spans(pay)
    assert s["kind"].tolist() == [Q, N, R, N, Q]
    assert s["flags"].tolist() == [7, 0, 7, 0, HM.HAS_LF | HM.HAS_TOKEN]
    assert s["method_len"].tolist() == [3, 0, 0, 0, 4]
    assert (s["tok_off"].tolist(), s["tok_len"].tolist()) == ([4, 0, 9, 0, 5], [2, 0, 3, 0, 0])
    assert (s["hdr_off"].tolist(), s["hdr_len"].tolist()) == ([17, 0, 16, 0, 15], [9, 0, 0, 0, 0])
    assert (s["body_off"].tolist(), s["body_len"].tolist()) == ([28, 0, 17, 0, 0], [4, 0, 0, 0, 0])
    assert HM.locate_stats(pay) == {"n_requests": 2, "n_responses": 1, "n_blank": 2, "bytes_scanned": len(pay[0]) + 3 + len(pay[2]) + 0 + len(pay[4])}
    w = HM.load_fields(pay, "raw_uri")
    assert w["payloads"] == [b"/a", b"", b"", b"", b""] and w["present"].tolist() == [True, False, False, False, True]
    assert w["off"].tolist() == [0, 16, 32, 48, 64] and w["len"].tolist() == [2, 0, 0, 0, 0] and len(w["arena"]) == 80
    assert w["stats"] == {"n_payloads": 5, "n_present": 2, "bytes_in": sum(map(len, pay)), "bytes_out": 2}
    w = HM.load_fields(pay, "raw_uri", only_present=True)
    assert w["payloads"] == [b"/a", b""] and w["index"].tolist() == [0, 4] and w["words"].tolist() == [0b10001]
    assert w["stats"] == {"n_payloads": 2, "n_present": 2, "bytes_in": len(pay[0]) + len(pay[4]), "bytes_out": 2}
    assert HM.load_fields(pay, "status", True)["payloads"] == [b"200"]


def test_bytes_scanned_steps():
    long_uri = b"GET /" + b"a" * 3000 + b" HTTP/1.1\r\n\r\n"
    assert HM.bytes_scanned(long_uri, HM.locate(long_uri)) == len(long_uri)                  # the blank line lies in the last step
    early = b"GET / HTTP/1.1\r\n\r\n" + b"b" * 5000
    assert HM.bytes_scanned(early, HM.locate(early)) == 1024                                 # one step
    no_blank = b"GET / HTTP/1.1\r\n" + b"h" * 5000
    assert HM.bytes_scanned(no_blank, HM.locate(no_blank)) == len(no_blank)                  # read to its end
    none_late = b"GET \n" + b"x" * 5000
    assert HM.locate(none_late)["kind"] == N and HM.bytes_scanned(none_late, HM.locate(none_late)) == 1024
    assert HM.bytes_scanned(b"\x00" * 100, HM.locate(b"\x00" * 100)) == 16 and HM.bytes_scanned(b"abc", HM.locate(b"abc")) == 3


# ------------------------------------------------------------------------------------------------
# the second formulation: regular expressions over bytes, no index arithmetic
# ------------------------------------------------------------------------------------------------
TOKENS = re.compile(rb"([^ ]*) (?=.)([^ ]*)", re.S)
REQUEST_LINE = re.compile(rb"[A-Z]{1,15} .", re.S)
BLANK = re.compile(rb"\n(?:\n|\r\n)")


def by_regex(p):
    head, lf, rest = p.partition(b"\n")
    line = head[:-1] if head.endswith(b"\r") else head
    if line.startswith(b"HTTP/"):
        kind = R
    elif REQUEST_LINE.match(line):
        kind = Q
    else:
        return N, (None,) * 5
    tok = TOKENS.match(line)
    method = tok.group(1) if kind == Q else None
    uri = tok.group(2) if kind == Q else None
    status = tok.group(2) if kind == R and tok else None
    headers = body = None
    if lf:
        m = BLANK.search(p)
        headers = p[len(head) + 1:m.start() + 1] if m else rest
        body = p[m.end():] if m else None
    return kind, (method, uri, status, headers, body)


ALPHABET = [b"A", b"G", b"e", b" ", b"\r", b"\n", b"H", b"T", b"P", b"/", b"1", b"x"]
PREFIXES = [b"", b"", b"", b"G ", b"GET ", b"GET /x", b"HTTP/", b"HTTP/1 ", b"AG /", b"GET /x HTTP/1\r\n", b"HTTP/1 1 x\n", b"TTP/"]


def random_strings(n, seed):
    rng = np.random.default_rng(seed)
    letters = rng.integers(0, len(ALPHABET), (n, 40))
    lens = rng.integers(0, 41, n)
    pre = rng.integers(0, len(PREFIXES), n)
    return [PREFIXES[pre[i]] + b"".join(ALPHABET[c] for c in letters[i, :lens[i]]) for i in range(n)]


def test_against_regex_formulation():
    strings = random_strings(100_000, 2029)
    kinds = np.zeros(3, dtype=np.int64)
    blank = 0
    for p in strings:
        got = fields(p)
        assert got == by_regex(p), p
        kinds[got[0]] += 1
        blank += got[1][4] is not None
    # agreement on a set that is all NONE would show nothing
    assert (kinds >= len(strings) // 20).all() and blank >= len(strings) // 20, (kinds.tolist(), blank)


@pytest.mark.parametrize("case", VERDICTS, ids=[repr(c[0])[:40] for c in VERDICTS])
def test_regex_formulation_on_verdicts(case):
    p, kind, *want = case
    assert by_regex(p) == (kind, tuple(want))
