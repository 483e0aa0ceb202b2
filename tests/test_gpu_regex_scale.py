"""The regex kernel (csrc/kmp_regex.hip) past its grid sizes, against tests/regex_model.py, exactly.  The periodic arenas are those of
tests/test_gpu_rows_scale.py: the model runs on one period of texts and numpy indexing expands its rows.

  kmp_regex_kernel: gridDim.x = ceil(stride / 4) blocks of four words; tile += gridDim.y, gridDim.y = min(tiles, 64, max(1, 1024 / gridDim.x)):
    past 1024 blocks in x a single block row takes every tile -- test_two_expressions_past_the_block_cap -- and with more tiles of
    KMP_RX_TILE expressions than gridDim.y a block stages a second tile behind its first write-out -- test_tiles_past_grid_y

Run on a real MI355X:  python -m pytest tests/test_gpu_regex_scale.py -m gpu
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import ONES, gm, reset  # noqa: E402,F401  (torch first; gm: the context fixture)

import match_model as MM  # noqa: E402
import regex_model as RM  # noqa: E402
from regex_model import rx  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from test_gpu_regex import _check  # noqa: E402
from test_gpu_rows_scale import N_BIG, N_HDR_Y3, SMALL_PATS, P, small  # noqa: E402

T = _lib.RX_TILE
RX_MAX_BY = 64                                              # RX_MAX_BY (kmp_regex.hip)
N_TILES = 3 * T + 1                                         # four tiles


def rx_grid(n_pkts, n_rx):
    """(gridDim.x, gridDim.y, tiles) of the regex kernel (kmp_launch_regexes)"""
    stride = ((n_pkts + 63) // 64 + 1) & ~1
    bx, tiles = (stride + 3) // 4, (n_rx + T - 1) // T
    return bx, min(tiles, RX_MAX_BY, max(1, 1024 // bx)), tiles


assert rx_grid(N_BIG, 2 * T)[:2] == (rx_grid(N_BIG, 2)[0], 1) and rx_grid(N_BIG, 2)[0] > 1024      # past the cap a block row takes every tile
assert rx_grid(N_HDR_Y3, N_TILES)[1:] == (3, 4) and N_TILES % T == 1                                # block y = 0 takes tiles 0 and 3


def _draw(texts, hits, n):
    """n expressions over the small alphabet, gated and ungated in turn, whose rows over the period's texts are neither empty nor full and
    differ from one another"""
    letters = [b"a", b"b", b"x", b"y", b"z", b"G", b"E", b"T", b"Q"]
    forms = [lambda a, b: a + b, lambda a, b: a + b"." + b, lambda a, b: b"^[^" + a + b"]*" + b + b"$", lambda a, b: b"[" + a + b + b"]{3,}",
             lambda a, b: a + b"+" + b + b"?$", lambda a, b: b"^.{0,5}" + a + b"[^" + b + b"]"]
    out, rows = [], []
    for i, ((a, b), form) in enumerate(itertools.product(itertools.permutations(letters, 2), forms)):
        if len(out) == n:
            break
        e = rx(form(a, b), nocase=bool(i % 3 == 0), gate=(len(out) % len(SMALL_PATS)) if len(out) % 2 else None)
        r = RM.regex_rows(texts, [e], False, hits)[0]
        if 0 < r[:P].sum() < P and not any(np.array_equal(r, o) for o in rows):
            out.append(e)
            rows.append(r)
    assert len(out) == n
    return out, np.array(rows)


def _raw_words(m, rows):
    """the bits at n_pkts and above are 0"""
    n_rx, n = rows.shape
    W = (n + 63) // 64
    hit_w, any_w = np.full((n_rx, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
    _lib.gpu_check(m._g.kmpgpu_scan_regexes(m._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_regexes")
    assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))


def test_two_expressions_past_the_block_cap(gm, oracle):
    s = small(N_BIG)
    text_hits = MM.hits(s.p.starts(SMALL_PATS), len(SMALL_PATS))
    exprs, text_rows = _draw(s.p.texts, text_hits, 2)
    rows = s.p.expand(text_rows)
    assert rows.shape == (2, N_BIG) and "gate" in exprs[1][1]
    try:
        reset(gm)
        s.load(gm)
        gm.set_regexes(exprs)
        _check(gm, rows, s.counts(oracle))
        _raw_words(gm, rows)
    finally:
        reset(gm)


def test_tiles_past_grid_y(gm, oracle):
    s = small(N_HDR_Y3)
    text_hits = MM.hits(s.p.starts(SMALL_PATS), len(SMALL_PATS))
    exprs, text_rows = _draw(s.p.texts, text_hits, N_TILES)
    rows = s.p.expand(text_rows)
    assert rows.shape == (N_TILES, N_HDR_Y3)
    assert all((rows[q] != rows[q + T]).any() for q in range(N_TILES - T))          # the rows of two tiles are never the same
    try:
        reset(gm)
        s.load(gm)
        gm.set_regexes(exprs)
        _check(gm, rows, s.counts(oracle))
        _raw_words(gm, rows)
        # as rule terms: an expression of the first tile and one of the last
        last = N_TILES - 1
        rules = [([gm.regex(last)], [0]), ([gm.regex(4)], [gm.regex(last)]), ([0], [gm.regex(2)])]
        gm.set_rules(rules)
        mat = np.concatenate([s.hits, rows])
        want = MM.rule_rows(mat, rules)
        assert want.any(axis=1).all() and not want.all(axis=1).any()
        got = gm.scan_rules(hits=True)
        assert np.array_equal(got["hits"], want) and got["rule_pkt_counts"].tolist() == want.sum(axis=1).tolist()
    finally:
        reset(gm)
