"""The byte-test kernels (csrc/kmp_bytetests.hip) past their grid sizes, against tests/bytetest_model.py, exactly.  The periodic arenas are
those of tests/test_gpu_rows_scale.py: the model runs on one period of texts and numpy indexing expands its rows.

  kmp_bytetests_rel_kernel: item += step, the grid capped at cu_count * 8 blocks of 4 wavefronts, one (relative test, word) each: a second and
    a third round from n_relative * W > PAIR_CAP on -- test_relative_tests_through_three_rounds
  kmp_bytetests_abs_kernel: tile += gridDim.y, gridDim.y = min(tiles, 64, max(1, 1024 / bx)), bx = ceil(stride / 4): more tiles of
    KMP_BT_TILE tests than gridDim.y, so that a block stages a second tile behind its first write-out -- test_absolute_tiles

Run on a real MI355X:  python -m pytest tests/test_gpu_bytetests_scale.py -m gpu
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import ONES, gm, reset  # noqa: E402,F401  (torch first; gm: the context fixture)

import bytetest_model as BM  # noqa: E402
import match_model as MM  # noqa: E402
from bytetest_model import bt  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.host import HostArena  # noqa: E402
from test_gpu_bytetests import _check  # noqa: E402
from test_gpu_rows_scale import (N_HDR_Y3, N_PAIR, PAIR_CAP, PAIR_LAST, PAIR_PATS, SMALL_PATS, W_PAIR, P, Periodic, _pair_classes,  # noqa: E402
                                 small)

U32 = 0xFFFFFFFF
BT_TILE = _lib.BT_TILE
BT_MAX_BY = 64                                              # BT_MAX_BY (kmp_bytetests.hip)
N_REL = (2 * PAIR_CAP + W_PAIR - 1) // W_PAIR + 3           # relative tests: a third round of (test, word) items
N_ABS = 3 * BT_TILE + 1                                     # four tiles


def abs_grid(n_pkts, n_bt):
    """(gridDim.y, tiles) of the absolute kernel (kmp_launch_bytetests)"""
    stride = ((n_pkts + 63) // 64 + 1) & ~1
    tiles = (n_bt + BT_TILE - 1) // BT_TILE
    return min(tiles, BT_MAX_BY, max(1, 1024 // ((stride + 3) // 4))), tiles


assert N_REL * W_PAIR > 2 * PAIR_CAP and (N_REL - 3) * W_PAIR <= 2 * PAIR_CAP + W_PAIR
assert abs_grid(N_HDR_Y3, N_ABS) == (3, 4) and N_ABS % BT_TILE == 1                     # block y = 0 takes tiles 0 and 3


def _field_of(rng, texts, nbytes, little):
    """a value that some text holds somewhere: compares on it split the texts"""
    t = rng.choice([t for t in texts if len(t) >= nbytes])
    s = rng.randrange(0, len(t) - nbytes + 1)
    return int.from_bytes(t[s:s + nbytes], "little" if little else "big")


def _draw(rng, texts, n, relative, pats):
    """n tests whose rows over the texts are neither empty nor full and differ from the row before"""
    out, rows = [], []
    st = MM.starts(texts, pats)
    while len(out) < n:
        nbytes, little = rng.randrange(1, 5), rng.random() < 0.5
        t = bt(nbytes, rng.randrange(6), _field_of(rng, texts, nbytes, little), rng.randrange(-8, 12) if relative else rng.randrange(0, 15),
               mask=rng.choice([U32, U32, 0xFF, 0x0F0F0F0F]), anchor=rng.randrange(len(pats)) if relative else None, little=little)
        r = BM.bytetest_rows(texts, pats, [t], st=st)[0]
        if 0 < r[:P].sum() < P and not (rows and np.array_equal(r, rows[-1])):
            out.append(t)
            rows.append(r)
    return out, np.array(rows)


def test_relative_tests_through_three_rounds(gm, oracle):
    p = Periodic(N_PAIR, _pair_classes(), b"", PAIR_LAST)
    tests, text_rows = _draw(random.Random("relative-rounds"), p.texts, N_REL, True, PAIR_PATS)
    rows = p.expand(text_rows)
    assert rows.shape == (N_REL, N_PAIR)
    items = MM.words(rows).reshape(-1)                       # item = relative test * W + word, as the kernel numbers them
    assert len(items) == N_REL * W_PAIR > 2 * PAIR_CAP
    for lo, hi in ((PAIR_CAP, 2 * PAIR_CAP), (2 * PAIR_CAP, len(items))):               # the second and the third round hold set and clear bits
        assert (items[lo:hi] != 0).any() and (items[lo:hi] != ONES).any() and len(set(items[lo:hi].tolist())) > 8
    counts = p.counts(oracle, PAIR_PATS)
    try:
        reset(gm)
        gm.set_patterns(PAIR_PATS)
        gm.load_arena(HostArena.from_payloads(p.payloads()))
        gm.set_bytetests(tests)
        res = _check(gm, rows, counts)
        assert res["timing"].launches == gm.scan_packets()["timing"].launches        # relative tests alone: one kernel
    finally:
        reset(gm)


def test_absolute_tiles(gm, oracle):
    s = small(N_HDR_Y3)
    rng = random.Random("absolute-tiles")
    tests, text_rows = _draw(rng, s.p.texts, N_ABS, False, SMALL_PATS)
    # a relative test in every tile, at a different place in each: its row is the other kernel's, and the tile's write-out passes over it
    for tile, at in enumerate((5, 77, 127, 0)):
        q = tile * BT_TILE + at
        rel, rel_rows = _draw(rng, s.p.texts, 1, True, SMALL_PATS)
        tests[q], text_rows[q] = rel[0], rel_rows[0]
    rows = s.p.expand(text_rows)
    assert rows.shape == (N_ABS, N_HDR_Y3)
    assert all((rows[q] != rows[q + BT_TILE]).any() for q in range(N_ABS - BT_TILE))        # the rows of two tiles are never the same
    counts = s.counts(oracle)
    try:
        reset(gm)
        s.load(gm)
        gm.set_bytetests(tests)
        _check(gm, rows, counts)
        # the raw words: the bits at n_pkts and above are 0
        W = (N_HDR_Y3 + 63) // 64
        hit_w, any_w = np.full((N_ABS, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
        _lib.gpu_check(gm._g.kmpgpu_scan_bytetests(gm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_bytetests")
        assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))
    finally:
        reset(gm)
