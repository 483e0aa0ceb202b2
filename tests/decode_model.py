"""The definition of kmpgpu_load_decoded (include/kmpgpu.h) in plain Python / numpy: what the GPU tests compare the library with, byte
for byte.  No device needed.

Every position of a payload is decided on its own: esc(i) = i + 2 < L and p[i] == '%' and p[i+1], p[i+2] hex digits; the decoded
payload takes the escape's byte where esc(i), nothing where esc(i-1) or esc(i-2), and p[i] otherwise (0x20 for a '+' with plus).
tests/test_decode_model.py holds this against urllib.parse.unquote_to_bytes."""
import numpy as np

HEX = np.zeros(256, dtype=bool)
HEX[list(b"0123456789abcdefABCDEF")] = True
VAL = np.zeros(256, dtype=np.uint8)
for _c in b"0123456789":
    VAL[_c] = _c - 0x30
for _c in b"abcdef":
    VAL[_c] = _c - 0x61 + 10
    VAL[_c - 0x20] = _c - 0x61 + 10

# the alphabet the transform is tried with: everything that can make, break or imitate an escape
HOSTILE = np.frombuffer(b"%0123456789abcdefABCDEFgG+/ \x00\xff", dtype=np.uint8)


def escapes(p: np.ndarray) -> np.ndarray:
    """esc(i) for every position of one payload (uint8 array)"""
    L = p.size
    e = np.zeros(L, dtype=bool)
    if L >= 3:
        e[:L - 2] = (p[:L - 2] == 0x25) & HEX[p[1:L - 1]] & HEX[p[2:]]
    return e


def decode(payload: bytes, plus: bool = False) -> bytes:
    p = np.frombuffer(payload, dtype=np.uint8)
    e = escapes(p)
    consumed = np.zeros(p.size, dtype=bool)
    consumed[1:] |= e[:-1]
    consumed[2:] |= e[:-2]
    out = p.copy()
    if plus:
        out[p == 0x2B] = 0x20
    i = np.flatnonzero(e)
    out[i] = 16 * VAL[p[i + 1]] + VAL[p[i + 2]]
    return out[~consumed].tobytes()


def changed(payload: bytes, plus: bool = False) -> bool:
    p = np.frombuffer(payload, dtype=np.uint8)
    return bool(escapes(p).any() or (plus and (p == 0x2B).any()))


def words(bits) -> np.ndarray:
    """bool[n] -> uint64[ceil(n / 64)], payload k = bit k & 63 of word k >> 6, the bits at n and above 0"""
    bits = np.asarray(bits, dtype=bool)
    W = (bits.size + 63) // 64
    b = np.zeros(W * 64, dtype=np.uint8)
    b[:bits.size] = bits
    return np.packbits(b, bitorder="little").view(np.uint64) if W else np.zeros(0, dtype=np.uint64)


def packed_image(payloads):
    """(arena bytes, offsets uint64, lengths uint32) of a packed arena: slots of max(16, round_up(len, 16)) bytes back to back from 0,
    0x00 behind every payload's end"""
    ln = np.array([len(t) for t in payloads], dtype=np.uint32)
    size = np.maximum(16, (ln.astype(np.uint64) + 15) & ~np.uint64(15))
    off = (np.cumsum(size) - size).astype(np.uint64)
    arena = np.zeros(int(size.sum()), dtype=np.uint8)
    for o, t in zip(off, payloads):
        arena[int(o):int(o) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return arena, off, ln


def load_decoded(payloads, plus: bool = False, only_changed: bool = False) -> dict:
    """What dst holds after kmpgpu_load_decoded over these payloads, and what the call hands out."""
    chg = np.array([changed(t, plus) for t in payloads], dtype=bool)
    index = np.flatnonzero(chg).astype(np.int64) if only_changed else np.arange(len(payloads), dtype=np.int64)
    out = [decode(payloads[int(k)], plus) for k in index]
    arena, off, ln = packed_image(out)
    return {"payloads": out, "arena": arena, "off": off, "len": ln, "changed": chg, "words": words(chg), "index": index,
            "stats": {"n_payloads": len(out), "n_changed": int(chg.sum()), "bytes_in": sum(len(payloads[int(k)]) for k in index),
                      "bytes_out": sum(len(t) for t in out)}}


def random_payload(rng, length: int) -> bytes:
    return HOSTILE[rng.integers(0, HOSTILE.size, length)].tobytes()


def escape_all(data: bytes) -> bytes:
    """every byte as its escape: the payload of maximum shrink"""
    return b"".join(b"%%%02X" % b if i & 1 else b"%%%02x" % b for i, b in enumerate(data))
