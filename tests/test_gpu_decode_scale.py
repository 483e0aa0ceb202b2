"""kmpgpu_load_decoded past every grid cap of csrc/kmp_decode.hip, on a real MI355X.

  kmp_decode_lengths_kernel   KMP_GRID_CAP 1 024 blocks * 4 wavefronts * 64 payloads: a second round past 262 144 payloads
  kmp_decode_index_kernel     KMP_GRID_CAP 1 024 * 256 threads: past 262 144 payloads
  kmp_scan_totals_kernel      one round of 256 block totals (kmp_prep.hip)
  kmp_decode_write_kernel     KMP_GRID_CAP 1 024 * 4 runs: past 4 096 runs -- runs of 64 payloads of 16..48 bytes (262 144
                              payloads), runs of 4 payloads of ~3 000 bytes (16 384 payloads)

The arenas are periodic: 257 distinct payloads with escapes, repeated.  tests/decode_model.py decodes the 257 once; what dst has to
hold -- index, lengths, offsets, every byte -- follows from the period by index arithmetic in numpy, and is compared exactly.

Run on a real MI355X:  python -m pytest tests/test_gpu_decode_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import reset  # noqa: E402  (torch first)

import decode_model as DM  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402
from test_gpu_decode import check_arena  # noqa: E402

PERIOD = 257
N_SMALL, N_LARGE = 300_001, 17_001
assert N_SMALL > 1024 * 4 * 64 and N_LARGE > 1024 * 4 * 4


@pytest.fixture(scope="module")
def src():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def dst():
    m = GpuMatcher(0)
    yield m
    m.close()


def period(kind):
    """257 distinct payloads: a third without anything to decode, the others with escapes -- also across unit and step boundaries -- and
    '+'; the last bytes of some an incomplete escape"""
    rng = np.random.default_rng(61 if kind == "small" else 62)
    out, seen = [], set()
    while len(out) < PERIOD:
        k = len(out)
        L = int(rng.integers(16, 49)) if kind == "small" else int(rng.integers(2900, 3101))
        t = bytearray(DM.random_payload(rng, L))
        if k % 3 == 0:
            t = bytearray(bytes(t).replace(b"%", b"x").replace(b"+", b"y"))
        else:
            for _ in range(1 + L // 200):
                i = int(rng.integers(0, L - 2))
                t[i:i + 3] = b"%%%02x" % int(rng.integers(0, 256))
            if k % 5 == 0:
                t[L - 2:] = b"%4"
        t = bytes(t)
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def tiled(per, reps, head):
    """`reps` whole periods of the packed image `per` = (arena, off, len), then its first `head` payloads"""
    arena, off, ln = per
    end = int(off[head]) if head < len(ln) else len(arena)
    return (np.concatenate([np.tile(arena, reps), arena[:end if head else 0]]), None, np.concatenate([np.tile(ln, reps), ln[:head]]))


def expectation(base, n, plus, only_changed):
    m = DM.load_decoded(base, plus, only_changed)
    reps, rest = divmod(n, PERIOD)
    head = int((m["index"] < rest).sum())                              # payloads of the last, incomplete period that dst holds
    arena, _, ln = tiled((m["arena"], m["off"], m["len"]), reps, head)
    slot = np.maximum(np.uint64(16), (ln.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15))
    index = np.concatenate([(np.arange(reps, dtype=np.int64)[:, None] * PERIOD + m["index"][None, :]).ravel(), reps * PERIOD + m["index"][:head]])
    changed = np.concatenate([np.tile(m["changed"], reps), m["changed"][:rest]])
    src_len = np.array([len(t) for t in base], dtype=np.int64)
    stats = {"n_payloads": len(ln), "n_changed": int(changed.sum()), "bytes_in": int(src_len[index % PERIOD].sum()), "bytes_out": int(ln.sum(dtype=np.uint64))}
    return {"arena": arena, "off": np.cumsum(slot) - slot, "len": ln, "index": index, "changed": changed, "stats": stats}


@pytest.fixture(scope="module", params=["small", "large"])
def source(request, src):
    kind = request.param
    base = period(kind)
    n = N_SMALL if kind == "small" else N_LARGE
    per = DM.packed_image(base)
    reps, rest = divmod(n, PERIOD)
    arena, _, ln = tiled(per, reps, rest)
    slot = np.maximum(np.uint64(16), (ln.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15))
    reset(src)
    src.load_arena(np.concatenate([arena, np.zeros(64, np.uint8)]), (np.cumsum(slot) - slot).astype(np.uint64), ln)
    assert src.arena_info() == (n, int(ln.sum(dtype=np.uint64)))
    return base, n


@pytest.mark.parametrize("plus, only_changed", [(False, False), (True, True)])
def test_at_scale(src, dst, source, plus, only_changed):
    base, n = source
    want = expectation(base, n, plus, only_changed)
    assert 0 < want["stats"]["n_changed"] < n
    try:
        reset(dst)
        res = dst.load_decoded(src, plus=plus, only_changed=only_changed)
        assert np.array_equal(res["changed"], want["changed"]) and np.array_equal(res["index"], want["index"])
        assert res["stats"] == want["stats"]
        check_arena(dst, want)
        assert dst.last_timing().launches == 5
    finally:
        reset(dst)
