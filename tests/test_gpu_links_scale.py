"""kmpgpu_link_rows past the gather's grid: more output words than the grid has wavefronts, so every wavefront takes a second word in its
grid-stride loop, and more map words than one tile of the rank kernel.  The launcher caps the grid at KMP_GRID_CAP blocks of
KMP_BLOCK_WAVES wavefronts; N is the first payload count whose words exceed twice that, plus an odd tail -- derived from the cap, not from a
workload.  One periodic arena of empty and 16-byte payloads, three rows, each map kind once, against tests/link_model.py."""
import os
import re

import numpy as np
import pytest

from gpu_support import PERIOD, PeriodicSource, periodic_end, torch  # noqa: F401  (before the package: gpu_support says why)

import link_model as LM
from multithreading_string_matching_amd.matcher import LINK_NONE, GpuMatcher

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "multithreading_string_matching_amd", "csrc", "kmp_launch.h")) as _f:
    _h = _f.read()
GRID_CAP = int(re.search(r"#define KMP_GRID_CAP\s+(\d+)u", _h).group(1))
RANK_TILE = int(re.search(r"#define KMP_LINK_RANK_TILE (\d+)u", _h).group(1))
GRID_WAVES = GRID_CAP * 4                          # KMP_BLOCK_WAVES = 256 / 64
# ... + 38: a tail word, and the last payload of the arena and of the shorter source (period entries 199 and 169) each hold a pattern
N = max(2 * GRID_WAVES * 64 + 64 + 38, 600_000 + 38)
PATS = [b"<A>", b"<B>", b"<C>"]
PAIRS = ((N + 63) // 64 + 1) // 2                  # 16-byte pairs of a row
SAME_ROWS = 2 * GRID_CAP * 256 // PAIRS + 2        # rows x pairs > 2 x (GRID_CAP blocks x KMP_BLOCK_THREADS)


def period_payloads():
    pay, holds = [], np.zeros((3, PERIOD), dtype=bool)
    for e in range(PERIOD):
        if e % 7 == 0:
            pay.append(b"")
            continue
        holds[:, e] = (e % 2 == 1, e % 3 == 1, e % 5 == 2)
        t = b"".join(p for p, h in zip(PATS, holds[:, e]) if h)
        pay.append(t + b"." * (16 - len(t)))
    return pay, holds


def test_every_map_kind_past_the_grid():
    assert N > GRID_WAVES * 64 and (N + 63) // 64 > RANK_TILE and N >= 600_000 and SAME_ROWS * PAIRS > 2 * GRID_CAP * 256
    pay, holds = period_payloads()
    rows_of = lambda n: holds[:, np.arange(n) % PERIOD]                      # noqa: E731
    rng = np.random.default_rng(11)
    n_src = N - 100_003
    bitmap = np.zeros(N, dtype=bool)
    bitmap[rng.permutation(N - 1)[:n_src - 1]] = True
    bitmap[-1] = True                                   # the last payload is mapped, to the source's last
    index = rng.integers(0, n_src + n_src // 8, N, dtype=np.int64)
    index[::97] = LINK_NONE
    index[-1] = n_src - 1
    index = index.astype(np.uint32)

    ps = PeriodicSource(PATS)
    dst = GpuMatcher(0)
    try:
        src = ps.build(pay, N)
        arena, off, ln = ps.keep
        dst.set_patterns([b"unused"])
        dst.attach_arena(arena, off, ln, arena_bytes=periodic_end(ps.image, N))
        dst.set_links(9)
        dst.link_rows(0, src, "patterns")
        src = ps.use(n_src)
        dst.link_rows(3, src, "patterns", map=bitmap)
        dst.link_rows(6, src, "patterns", map=index)
        got = dst.scan_links(hits=True)
        want = np.concatenate([LM.link(rows_of(N), N, N, LM.SAME), LM.link(rows_of(n_src), n_src, N, LM.BITMAP, bitmap),
                               LM.link(rows_of(n_src), n_src, N, LM.INDEX, index)])
        for q in range(9):
            bad = np.flatnonzero(got["hits"][q] != want[q])
            assert bad.size == 0, (q, bad.size, bad[:8].tolist())
        assert got["link_pkt_counts"].tolist() == want.sum(axis=1).tolist()
        assert np.array_equal(got["any"], want.any(axis=0))
        assert want[0, -1] and want[3, -1] and want[6, -1] and want.sum() > N
        # the identity copy past ITS grid: SAME_ROWS rows of N payloads are more 16-byte pairs than GRID_CAP blocks of 256 threads hold,
        # so every thread of kmp_link_same_kernel takes a second item.  The rows are rules of src.
        src = ps.use(N)
        src.set_rules([([q % 3], []) if q % 2 else ([q % 3], [(q + 1) % 3]) for q in range(SAME_ROWS)])
        dst.set_links(SAME_ROWS)
        dst.link_rows(0, src, "rules")
        base = rows_of(N)
        want = np.stack([base[q % 3] if q % 2 else base[q % 3] & ~base[(q + 1) % 3] for q in range(SAME_ROWS)])
        got = dst.scan_links(hits=True)
        assert np.array_equal(got["hits"], want)
        assert got["link_pkt_counts"].tolist() == want.sum(axis=1).tolist() and want[-1].any() and want[:, -1].any()
    finally:
        dst.close()
        ps.close()
