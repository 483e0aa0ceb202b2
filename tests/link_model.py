"""The definition of kmpgpu_link_rows in numpy: rows of one context in another context's payload numbering.  No device needed.

link(rows_src, n_src, n_dst, kind, map) -> bool[R, n_dst]: bit k of an output row is bit map(k) of the source row where k < n_dst,
map(k) exists and map(k) < n_src; every other bit is 0.
  SAME    map(k) = k; n_src must equal n_dst; map is not looked at.
  BITMAP  map: uint64 words (or bool[>= n_dst]); the j-th set bit below n_dst is the source's payload j.  Bits at n_dst and above are
          ignored; a popcount below n_dst that is not n_src is a ValueError (the library's KMPGPU_EINVAL).
  INDEX   map: uint32[n_dst], the source's payload for every payload; a value >= n_src (NONE among them): none.
"""
import numpy as np

SAME, BITMAP, INDEX = 0, 1, 2
NONE = 0xFFFFFFFF


def bitmap_bits(map, n_dst):
    """bool[n_dst] of a bitmap map given as uint64 words or as bools"""
    map = np.asarray(map)
    if map.dtype == np.bool_:
        bits = map
    else:
        bits = np.unpackbits(np.ascontiguousarray(map, dtype=np.uint64).view(np.uint8), bitorder="little").astype(bool)
    if len(bits) < n_dst:
        raise ValueError(f"bitmap of {len(bits)} bits for {n_dst} payloads")
    return bits[:n_dst]


def source_index(n_src, n_dst, kind, map):
    """int64[n_dst]: map(k), or -1 where payload k has no source payload"""
    if kind == SAME:
        if n_src != n_dst:
            raise ValueError(f"SAME between {n_src} and {n_dst} payloads")
        return np.arange(n_dst, dtype=np.int64)
    if kind == BITMAP:
        bits = bitmap_bits(map, n_dst)
        if int(bits.sum()) != n_src:
            raise ValueError(f"the bitmap has {int(bits.sum())} bits below {n_dst}, the source holds {n_src} payloads")
        return np.where(bits, np.cumsum(bits) - 1, -1).astype(np.int64)
    if kind == INDEX:
        idx = np.asarray(map)
        if idx.dtype != np.uint32 or idx.shape != (n_dst,):
            raise ValueError(f"index map {idx.dtype}{list(idx.shape)} for {n_dst} payloads")
        idx = idx.astype(np.int64)
        return np.where(idx < n_src, idx, -1)
    raise ValueError(f"map kind {kind}")


def link(rows_src, n_src, n_dst, kind, map=None):
    rows_src = np.atleast_2d(np.asarray(rows_src, dtype=bool))
    if rows_src.shape[1] != n_src:
        raise ValueError(f"rows of {rows_src.shape[1]} bits for {n_src} payloads")
    s = source_index(n_src, n_dst, kind, map)
    out = np.zeros((rows_src.shape[0], n_dst), dtype=bool)
    has = s >= 0
    out[:, has] = rows_src[:, s[has]]
    return out
