"""A numpy model of what the arena-building kernels (csrc/kmp_prep.hip) have to produce.

Plain helper of tests/test_prep_model.py (which holds it to the host library and the CPU oracle) and of
tests/test_gpu_prep_scale.py (which holds the kernels to it).  Nothing here touches a GPU.

``kmpgpu_load_frames`` only asks that every (frame_off, frame_caplen) lies inside the file buffer, so a test hands it a small
LIBRARY of distinct frames and an index of millions of entries that point into it.  What has to come out follows from
numpy alone:

* per library frame ("kind") the accept / reject rule gives (payload offset, payload length) or "rejected" -- taken from the CPU
  oracle (``library_rule``), never from the code under test;
* for a sequence ``kind[0..n)``: the accepted entries in order, ``pkt_len = plen[kind]``, ``slot = max(16, round_up(len, 16))``,
  ``pkt_off`` = exclusive cumsum of the slots, arena = every payload followed by 0x00 up to its slot's end (``gather_slots``).

Payloads of 8 bytes or more that the generator makes on purpose start with a tag ``<K00042>`` (the kind's number), the rest is
lower-case filler, so the number of times a tag is found in an arena pins every payload to its source (``tag_counts``).
"""
import random
import re
import struct

import numpy as np

REJECTED = -1
ROUND_ITEMS = 262144            # items one round of kmp_scan_totals_kernel covers: 256 tiles of 1024 (see tests/test_gpu_prep_scale.py)

# payload lengths around every multiple of the 16-byte slot, and past one 64-lane step of the gather (256 bytes)
PAYLOAD_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300]
BIG_LENGTHS = [1458, 8958]
_FILL = b"abcdefghijklmnopqrstuvwxyz"
_TAG = re.compile(rb"<K(\d{5})>")


def tag(k):
    return b"<K%05d>" % k


def slot_bytes(ln):
    """max(16, round_up(len, 16)) of every length, uint64."""
    ln = np.asarray(ln, dtype=np.uint64)
    return np.maximum(np.uint64(16), (ln + np.uint64(15)) & ~np.uint64(15))


def _payload(rng, kind, L):
    body = bytes(rng.choice(_FILL) for _ in range(L))
    return tag(kind) + body[8:] if L >= 8 else body


def _eth():
    return bytes(range(1, 13)) + b"\x08\x00"


def _ip(rng, ihl, proto, total):
    h = bytearray(rng.randrange(256) for _ in range(4 * ihl))
    h[0] = 0x40 | ihl
    h[2:4] = struct.pack(">H", total & 0xFFFF)
    h[9] = proto
    return bytes(h)


def udp_frame(rng, kind, ihl, L):
    return _eth() + _ip(rng, ihl, 17, 4 * ihl + 8 + L) + struct.pack(">HHHH", 1000 + kind % 1000, 53, 8 + L, 0) + _payload(rng, kind, L)


def tcp_frame(rng, kind, ihl, doff, L):
    t = bytearray(rng.randrange(256) for _ in range(4 * doff))
    t[12] = (doff << 4) | (t[12] & 0x0F)
    return _eth() + _ip(rng, ihl, 6, 4 * ihl + 4 * doff + L) + bytes(t) + _payload(rng, kind, L)


def frame_library(seed=7):
    """A few hundred distinct frames: UDP with IHL 5 / 6 / 15, TCP with header lengths 20..60, frames cut short at and around every
    header boundary (and two at every length), random bytes, a few payloads of 1 458 and 8 958 bytes.  A frame's position in the
    list is its kind."""
    rng = random.Random(seed)
    frames = []
    for ihl in (5, 6, 15):
        for L in PAYLOAD_LENGTHS:
            frames.append(udp_frame(rng, len(frames), ihl, L))
    for ihl in (5, 6):
        for doff in range(5, 16):
            for j in range(4):
                L = PAYLOAD_LENGTHS[(7 * doff + 3 * j + ihl) % len(PAYLOAD_LENGTHS)]
                frames.append(tcp_frame(rng, len(frames), ihl, doff, L))
    for L in BIG_LENGTHS:
        for ihl in (5, 6, 15):
            frames.append(udp_frame(rng, len(frames), ihl, L))
        for doff in (5, 8, 15):
            frames.append(tcp_frame(rng, len(frames), 5, doff, L))
    # cut short: at, one before and one behind every header boundary ...
    for ihl in (5, 6, 15):
        full = udp_frame(rng, len(frames), ihl, 33)
        ip_end = 14 + 4 * ihl
        for cut in sorted({0, 1, 13, 14, 15, 23, 24, 33, 34, 35, ip_end - 1, ip_end, ip_end + 1, ip_end + 7, ip_end + 8, ip_end + 9, len(full) - 1}):
            frames.append(full[:cut])
    for ihl, doff in ((5, 5), (5, 8), (6, 15), (15, 15)):
        full = tcp_frame(rng, len(frames), ihl, doff, 33)
        ip_end, tcp_end = 14 + 4 * ihl, 14 + 4 * ihl + 4 * doff
        for cut in sorted({0, 14, 15, 16, 33, 34, ip_end - 1, ip_end, ip_end + 12, ip_end + 13, ip_end + 14, ip_end + 19, ip_end + 20, tcp_end - 1, tcp_end,
                           tcp_end + 1, len(full) - 1}):
            frames.append(full[:cut])
    # ... and at every length
    for full in (udp_frame(rng, len(frames), 6, 20), tcp_frame(rng, len(frames), 5, 6, 20)):
        for cut in range(len(full)):
            frames.append(full[:cut])
    # random bytes, nudged towards the fields the rules read (NUL bytes included: they end what a scan counts)
    for _ in range(150):
        n = rng.randrange(0, 130)
        f = bytearray(rng.randrange(256) for _ in range(n))
        if n > 23 and rng.random() < 0.6:
            f[23] = 17
        if n > 14 and rng.random() < 0.7:
            f[14] = 0x40 | rng.choice([0, 4, 5, 5, 5, 6, 15])
        if n > 46 and rng.random() < 0.5:
            f[46] = rng.choice([0x40, 0x50, 0x50, 0x80, 0xF0])
        frames.append(bytes(f))
    return frames


def library_blob(frames):
    """The frames back to back (so most start unaligned): (bytes u8, offset u64[K], caplen u32[K])."""
    cap = np.array([len(f) for f in frames], dtype=np.uint32)
    off = np.zeros(len(frames), dtype=np.uint64)
    off[1:] = np.cumsum(cap[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(frames) + b"\0", dtype=np.uint8)[:-1].copy(), off, cap


def library_rule(frames, proto, dump):
    """(payload offset, payload length) of every kind as int64 arrays, length REJECTED where the rule drops the frame.
    dump(frame, caplen, proto) -> (off, len) or None: oracle.dump, or the host library's extract."""
    poff = np.zeros(len(frames), dtype=np.int64)
    plen = np.full(len(frames), REJECTED, dtype=np.int64)
    for k, f in enumerate(frames):
        r = dump(f, len(f), proto)
        if r is not None:
            poff[k], plen[k] = r
    return poff, plen


def library_payloads(frames, poff, plen):
    return [None if plen[k] < 0 else f[int(poff[k]):int(poff[k] + plen[k])] for k, f in enumerate(frames)]


def gather_slots(src, src_off, ln, chunk=65536):
    """The packed arena of payloads src[src_off[k] : +ln[k]] in index order: (pkt_off u64[n], arena u8 up to the last slot's
    end).  Every payload is followed by 0x00 up to the end of its slot.  Built in chunks of `chunk` payloads."""
    src = np.asarray(src, dtype=np.uint8)
    src_off = np.asarray(src_off, dtype=np.int64)
    ln = np.asarray(ln, dtype=np.int64)
    slot = slot_bytes(ln).astype(np.int64)
    off = np.zeros(len(ln), dtype=np.int64)
    if len(ln) > 1:
        off[1:] = np.cumsum(slot[:-1])
    total = int(off[-1] + slot[-1]) if len(ln) else 0
    arena = np.zeros(total, dtype=np.uint8)
    last = max(len(src) - 1, 0)
    for lo in range(0, len(ln), chunk):
        hi = min(lo + chunk, len(ln))
        d0, d1 = int(off[lo]), int(off[hi - 1] + slot[hi - 1])
        pos = np.arange(d0, d1, dtype=np.int64) - np.repeat(off[lo:hi], slot[lo:hi])        # byte's position in its slot
        idx = np.minimum(np.repeat(src_off[lo:hi], slot[lo:hi]) + pos, last)
        seg = src[idx] if len(src) else np.zeros(d1 - d0, np.uint8)
        seg[pos >= np.repeat(ln[lo:hi], slot[lo:hi])] = 0
        arena[d0:d1] = seg
    return off.astype(np.uint64), arena


def clean_padding(arena, off, ln, chunk=65536):
    """A copy of `arena` with the bytes between every payload's end and its slot's end put to 0x00 (slots may lie anywhere)."""
    out = np.array(arena, dtype=np.uint8, copy=True)
    off = np.asarray(off, dtype=np.int64)
    ln = np.asarray(ln, dtype=np.int64)
    pad = slot_bytes(ln).astype(np.int64) - ln
    for lo in range(0, len(ln), chunk):
        hi = min(lo + chunk, len(ln))
        p = pad[lo:hi]
        start = np.repeat(off[lo:hi] + ln[lo:hi], p)
        first = np.repeat(np.cumsum(p) - p, p)
        out[start + (np.arange(int(p.sum()), dtype=np.int64) - first)] = 0
    return out


def extraction_index(blob_off, poff, plen, kind):
    """What kmpgpu_load_frames has to leave for the frame sequence `kind`, without the bytes: (kinds of the accepted entries in
    order, pkt_off u64, pkt_len u32, where every payload starts in the library).  blob_off / poff / plen: per kind, from
    library_blob and library_rule."""
    kind = np.asarray(kind, dtype=np.int64)
    acc = kind[plen[kind] >= 0]
    ln = plen[acc].astype(np.uint32)
    return acc, packed_offsets(ln), ln, np.asarray(blob_off).astype(np.int64)[acc] + poff[acc]


def extraction_arena(blob, blob_off, poff, plen, kind):
    """(accepted kinds, pkt_off, pkt_len, arena bytes up to the last slot's end)."""
    acc, _, ln, src_off = extraction_index(blob_off, poff, plen, kind)
    off, arena = gather_slots(blob, src_off, ln)
    return acc, off, ln, arena


def packed_offsets(ln):
    slot = slot_bytes(ln)
    off = np.zeros(len(slot), dtype=np.uint64)
    if len(slot) > 1:
        off[1:] = np.cumsum(slot[:-1], dtype=np.uint64)
    return off


def effective_bytes(arena, off, ln):
    """Sum over payloads of min(len, first 0x00 + 1): what kmpgpu_effective_bytes reports."""
    off = np.asarray(off, dtype=np.int64)
    ln = np.asarray(ln, dtype=np.int64)
    z = np.flatnonzero(np.asarray(arena) == 0)
    if len(z) == 0:
        return int(ln.sum())
    j = np.searchsorted(z, off)
    first = np.where(j < len(z), z[np.minimum(j, len(z) - 1)], np.iinfo(np.int64).max)
    return int(np.where(first < off + ln, first - off + 1, ln).sum())


def tag_counts(payloads, acc, n_kinds):
    """counts[t] = how often tag(t) is found by a scan of the arena whose payloads are the kinds `acc`: occurrences in a kind's
    payload before its first 0x00, times how often the kind was accepted."""
    times = np.bincount(acc, minlength=n_kinds)
    want = np.zeros(n_kinds, dtype=np.uint64)
    for k, p in enumerate(payloads):
        if p is None or not times[k]:
            continue
        for m in _TAG.finditer(p.split(b"\0")[0]):
            if int(m.group(1)) < n_kinds:
                want[int(m.group(1))] += np.uint64(times[k])
    return want


def own_tag_kinds(payloads):
    """Kinds whose payload holds the kind's own tag exactly once and no other kind's payload holds it: for these
    count(tag) == number of accepted entries of the kind, whatever the sequence."""
    seen = {}
    for k, p in enumerate(payloads):
        if p is None:
            continue
        for m in _TAG.finditer(p.split(b"\0")[0]):
            seen.setdefault(int(m.group(1)), []).append(k)
    return [t for t, ks in sorted(seen.items()) if ks == [t]]


def make_sequence(shape, n, plen, seed):
    """A frame sequence of n kinds.  mixed: uniform over the library; all_rejected; last_only / first_only: one accepted entry;
    empty_rounds: whole rounds of ROUND_ITEMS entries rejected between mixed ones (two of every three, the first and the last
    round kept mixed); all_empty: accepted payloads of length 0 only, rejected frames between them."""
    rng = np.random.default_rng(seed)
    K = len(plen)
    rej = np.flatnonzero(plen < 0)
    good = np.flatnonzero(plen > 0)
    if shape == "mixed":
        return rng.integers(0, K, n)
    if shape == "all_rejected":
        return rej[rng.integers(0, len(rej), n)]
    if shape in ("last_only", "first_only"):
        kind = rej[rng.integers(0, len(rej), n)]
        kind[-1 if shape == "last_only" else 0] = good[int(rng.integers(0, len(good)))]
        return kind
    if shape == "empty_rounds":
        kind = rng.integers(0, K, n)
        rounds = (n + ROUND_ITEMS - 1) // ROUND_ITEMS
        for r in range(1, rounds - 1):
            if r % 3:
                lo, hi = r * ROUND_ITEMS, min(n, (r + 1) * ROUND_ITEMS)
                kind[lo:hi] = rej[rng.integers(0, len(rej), hi - lo)]
        return kind
    if shape == "all_empty":
        pool = np.concatenate([np.flatnonzero(plen == 0), rej[:3]])
        return pool[rng.integers(0, len(pool), n)]
    raise ValueError(shape)


def write_pcap(path, frames, kind):
    """A classic little-endian pcap whose records are frames[kind[0]], frames[kind[1]], ..."""
    recs = [struct.pack("<IIII", 0, 0, len(f), len(f)) + f for f in frames]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 262144, 1))
        fh.write(b"".join(recs[int(k)] for k in kind))


def shuffled_arena(n, seed, max_len=120, nul_permille=5):
    """A caller's arena that is legal but not packed: n payloads of 0..max_len bytes over {a, b, c} with `nul_permille` per mille
    0x00 bytes, slots in shuffled order with random gaps of 0..48 bytes (multiples of 16) between them, the gaps and the slot
    padding filled with 'b'.  Returns (arena u8, off u64, len u32)."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, max_len + 1, n).astype(np.int64)
    slot = slot_bytes(ln).astype(np.int64)
    order = rng.permutation(n)
    gap = 16 * rng.integers(0, 4, n)
    adv = gap + slot[order]
    start = np.cumsum(adv) - slot[order]
    off = np.zeros(n, dtype=np.int64)
    off[order] = start
    nbytes = int(adv.sum()) + 64
    text = rng.integers(ord("a"), ord("c") + 1, nbytes).astype(np.uint8)
    text[rng.random(nbytes) < nul_permille / 1000.0] = 0
    arena = np.full(nbytes, ord("b"), dtype=np.uint8)
    _, packed = gather_slots(text, off, ln)                        # payload k = text[off[k] : +ln[k]], computed once, packed
    poff = packed_offsets(ln).astype(np.int64)
    for lo in range(0, n, 65536):                                  # ... and laid out at the shuffled offsets
        hi = min(lo + 65536, n)
        l = ln[lo:hi]
        first = np.repeat(np.cumsum(l) - l, l)
        pos = np.arange(int(l.sum()), dtype=np.int64) - first
        arena[np.repeat(off[lo:hi], l) + pos] = packed[np.repeat(poff[lo:hi], l) + pos]
    return arena, off.astype(np.uint64), ln.astype(np.uint32)
