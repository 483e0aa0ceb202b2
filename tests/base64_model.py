"""The definition of kmpgpu_load_base64 (include/kmpgpu.h) in plain Python / numpy: what the GPU tests compare the library with, byte
for byte.  No device needed.

Written position by position, as the header states it: the maximal runs of alphabet bytes inside the payload, the runs of min_run and
more decoded (run offset r: nothing where r % 4 == 0, otherwise one byte made of p[i-1] and p[i]), up to two / one '=' directly behind
a decoded run of m % 4 == 2 / 3 dropped, every other byte copied.  tests/test_base64_model.py holds this against re + base64."""
import base64
import re

import numpy as np

from decode_model import packed_image, words  # noqa: F401  (the arena image and the bitmap words are the same)

STD = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
URL = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"


def _tables(urlsafe: bool):
    chars = URL if urlsafe else STD
    alpha = np.zeros(256, dtype=bool)
    val = np.zeros(256, dtype=np.uint32)
    for v, c in enumerate(chars):
        alpha[c] = True
        val[c] = v
    return alpha, val


TABLES = {False: _tables(False), True: _tables(True)}

# what the transform is tried with: alphabet bytes of both alphabets, '=' three times so that padding is common, and what ends a run
HOSTILE = np.frombuffer(b"AQgz09+/-_=== .:%\x00\xff\r\n", dtype=np.uint8)


def runs(payload: bytes, urlsafe: bool = False):
    """the maximal alphabet runs of one payload: (s int64[], e int64[])"""
    alpha, _ = TABLES[bool(urlsafe)]
    a = np.concatenate([[False], alpha[np.frombuffer(payload, dtype=np.uint8)], [False]]).astype(np.int8)
    d = np.diff(a)
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


def decode(payload: bytes, min_run: int, urlsafe: bool = False) -> bytes:
    assert 4 <= min_run <= 255
    _, val = TABLES[bool(urlsafe)]
    p = np.frombuffer(payload, dtype=np.uint8)
    L = p.size
    keep = np.ones(L, dtype=bool)           # the position yields a byte
    out = p.copy()                          # ... this one
    s, e = runs(payload, urlsafe)
    for s, e in zip(s[e - s >= min_run], e[e - s >= min_run]):
        s, e = int(s), int(e)
        i = np.arange(s, e)
        r = (i - s) % 4
        keep[i[r == 0]] = False
        j = i[r != 0]
        rj = r[r != 0]
        out[j] = ((val[p[j - 1]] << (2 * rj)) | (val[p[j]] >> (6 - 2 * rj))) & 0xFF
        pads = {2: 2, 3: 1}.get((e - s) % 4, 0)
        i = e
        while pads and i < L and p[i] == 0x3D:
            keep[i] = False
            pads -= 1
            i += 1
    return out[keep].tobytes()


def changed(payload: bytes, min_run: int, urlsafe: bool = False) -> bool:
    s, e = runs(payload, urlsafe)
    return bool((e - s >= min_run).any())


def decode_re(payload: bytes, min_run: int, urlsafe: bool = False) -> bytes:
    """the same through re + base64, run by run (the second formulation of the issue and the header)"""
    cls = rb"[A-Za-z0-9\-_]" if urlsafe else rb"[A-Za-z0-9+/]"
    dec = base64.urlsafe_b64decode if urlsafe else base64.b64decode

    def one(mt):
        run, eq = mt.group(1), mt.group(2)
        m = len(run)
        if m % 4 == 1:
            run = run[:-1]
        used = min(len(eq), {2: 2, 3: 1}.get(m % 4, 0))
        return dec(run + b"=" * (-len(run) % 4)) + eq[used:]

    return re.sub(rb"(" + cls + rb"{%d,})(={0,2})" % min_run, one, payload)


def load_base64(payloads, min_run: int = 16, urlsafe: bool = False, only_changed: bool = False) -> dict:
    """What dst holds after kmpgpu_load_base64 over these payloads, and what the call hands out."""
    chg = np.array([changed(t, min_run, urlsafe) for t in payloads], dtype=bool)
    index = np.flatnonzero(chg).astype(np.int64) if only_changed else np.arange(len(payloads), dtype=np.int64)
    out = [decode(payloads[int(k)], min_run, urlsafe) for k in index]
    arena, off, ln = packed_image(out)
    return {"payloads": out, "arena": arena, "off": off, "len": ln, "changed": chg, "words": words(chg), "index": index,
            "stats": {"n_payloads": len(out), "n_changed": int(chg.sum()), "bytes_in": sum(len(payloads[int(k)]) for k in index),
                      "bytes_out": sum(len(t) for t in out)}}


def random_payload(rng, length: int) -> bytes:
    return HOSTILE[rng.integers(0, HOSTILE.size, length)].tobytes()


def encode(data: bytes, urlsafe: bool = False, pad: bool = True) -> bytes:
    t = base64.urlsafe_b64encode(data) if urlsafe else base64.b64encode(data)
    return t if pad else t.rstrip(b"=")
