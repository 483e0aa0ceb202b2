"""The grouped regex kernel (kmp_regex_groups.hip) past its grid sizes, on the periodic arenas of tests/test_gpu_rows_scale.py:

  x    more than 1 024 blocks in x (N_BIG payloads: 2 065 blocks), where gridDim.y falls to 1: two flagged expressions, one tile
  x3   the same arena with 2 KMP_RXG_TILE + 1 flagged expressions among unflagged ones: one block walks three tiles
  y3   N_HDR_Y3 payloads (257 blocks in x, gridDim.y = 3) and 3 KMP_RXG_TILE + 1 flagged expressions: block y = 0 takes tiles 0 and 3

so the tile loop runs again in one block -- the barrier at its top, the reload of the tile behind a write-out, any[] carried across tiles --
and rows, counts, any[] and the raw words are compared with tests/regex_model.py over the arena's texts."""
import numpy as np
import pytest

from gpu_support import ONES, gm, reset  # noqa: F401  (gm: the context fixture)

import match_model as MM
import regex_model as RM
from multithreading_string_matching_amd import _lib
from test_gpu_rows_scale import N_BIG, N_HDR_Y3, SMALL_PATS, small

pytestmark = pytest.mark.gpu

TG = _lib.RXG_TILE
RXG_MAX_BY = 64                       # RXG_MAX_BY (kmp_regex_groups.hip)

# over the texts of the small arena: bytes of "abxyzGETQ", a 0x00 in a few, at most 16 bytes
FLAGGED = [b"(GET|xyz)", b"(a|b)(x|y)", b"^(a|b|x|y)+$", b"(Q|zz)(a|G)?(b|E)", b"(ab|ba|zz){1,2}(x|Q)", b"(?:E|T)(T|a)+", b"(x|y)z|Qa",
           b"((a|b|x)(y|z|a)){1,2}", b"^(G|x)", b"(a|z)$", b"(yz|ET)(\\x00|Q)", b"(G(E|a)|b(a|y))T?(x|b)", b"(a|b|G){3,}"]
LINEAR = [b"[ab]x", b"^[a-z]+$", b"GET", b"Q.?z", b"[xyz]{3}", b"T$"]


def groups_grid(n_pkts, n_groups):
    """(gridDim.x, gridDim.y, tiles) of kmp_launch_regex_groups"""
    stride = ((n_pkts + 63) // 64 + 1) & ~1
    bx, tiles = (stride + 3) // 4, (n_groups + TG - 1) // TG
    return bx, min(tiles, RXG_MAX_BY, max(1, 1024 // bx)), tiles


assert groups_grid(N_BIG, 2)[:2] == (2065, 1) and groups_grid(N_BIG, 2 * TG + 1) == (2065, 1, 3)
assert groups_grid(N_HDR_Y3, 3 * TG + 1) == (257, 3, 4) and len(FLAGGED) == 3 * TG + 1


def _flag(e, gate=None):
    return (e, {"groups": True} if gate is None else {"groups": True, "gate": gate})


def _model(x):
    """the expression as the model takes it: `groups` is the library's business alone"""
    expr, opt = (x, {}) if isinstance(x, bytes) else x
    return (expr, {k: v for k, v in opt.items() if k != "groups"})


def _sets():
    two = [_flag(FLAGGED[0]), _flag(FLAGGED[1], gate=1)]
    mixed = []
    for i in range(2 * TG + 1):                              # flagged and unflagged taking turns, every third flagged one gated
        mixed.append(_flag(FLAGGED[i], gate=i % len(SMALL_PATS)) if i % 3 == 2 else _flag(FLAGGED[i]))
        if i < len(LINEAR):
            mixed.append(LINEAR[i])
    every = [_flag(e, gate=0) if i == 5 else _flag(e) for i, e in enumerate(FLAGGED)]
    return {"x": (N_BIG, two), "x3": (N_BIG, mixed), "y3": (N_HDR_Y3, every)}


@pytest.mark.parametrize("case", ["x", "x3", "y3"])
def test_grouped_kernel_past_its_grid(gm, case):
    n, exprs = _sets()[case]
    s = small(n)
    text_hits = MM.hits(s.p.starts(SMALL_PATS), len(SMALL_PATS))
    text_rows = RM.regex_rows(s.p.texts, [_model(x) for x in exprs], False, text_hits)
    free = RM.regex_rows(s.p.texts, [_model(x)[0] for x in exprs], False, text_hits)
    assert all(0 < r.sum() < len(s.p.texts) for r in free), free.sum(axis=1).tolist()
    assert text_rows.any(axis=1).sum() >= len(exprs) - 1 and (text_rows != free).any()       # a gate takes something away
    rows = s.p.expand(text_rows)
    reset(gm)
    try:
        s.load(gm)
        gm.set_regexes(exprs)
        res = gm.scan_regexes(hits=True)
        assert np.array_equal(res["hits"], rows), np.argwhere(res["hits"] != rows)[:8].tolist()
        assert res["rx_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
        assert np.array_equal(res["any"], rows.any(axis=0))
        W = (n + 63) // 64
        rc, any_w, hit_w = np.full(len(exprs), 7, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64), np.full((len(exprs), W), ONES, dtype=np.uint64)
        _lib.gpu_check(gm._g.kmpgpu_scan_regexes(gm._ctx, rc.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_regexes")
        assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))
        assert rc.tolist() == rows.sum(axis=1).tolist()
    finally:
        reset(gm)
