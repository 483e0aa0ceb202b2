"""kmpgpu_load_base64 past every grid cap of csrc/kmp_base64.hip, and writing an arena across and behind offset 2^32, on a real MI355X.

  kmp_base64_lengths_kernel   KMP_GRID_CAP 1 024 blocks * 4 wavefronts * 64 payloads: a second round past 262 144 payloads
  kmp_decode_index_kernel     KMP_GRID_CAP 1 024 * 256 threads: past 262 144 payloads (kmp_decode.hip, shared)
  kmp_scan_totals_kernel      one round of 256 block totals (kmp_prep.hip)
  kmp_base64_write_kernel     KMP_GRID_CAP 1 024 * 4 runs: past 4 096 runs -- runs of 64 payloads of 16..48 bytes (262 144
                              payloads), runs of 4 payloads of ~3 000 bytes (16 384 payloads)

The arenas are periodic: 257 distinct payloads with base64 runs, repeated.  tests/base64_model.py decodes the 257 once; what dst has to
hold -- index, lengths, offsets, every byte -- follows from the period by index arithmetic in numpy, and is compared exactly.

The destination past 2^32 is built the way tests/test_gpu_high_destinations.py builds its own (its helpers are imported, the file is as
it was): the source laid out on the device by torch and borrowed in place, every payload under its tag `<K00123>` -- a run of six, so it
survives min_run = 16 --, the downloaded arena compared by one reshape against the period's image, and the 257 tags counted over dst.
Address arithmetic read before the first run: kmp_base64_write_kernel takes doff uint64 from LDS, d = doff + before, out = doff + before,
a0 = bcast64(out, 0) & ~15ull, pos = (uint32_t)(out - a0), d = a0 + 16ull * t, every guard d + 16 <= total in 64 bits -- the lines of
kmp_decode_write_kernel.

Run on a real MI355X:  python -m pytest tests/test_gpu_base64_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import B32, PERIOD, periodic_dst, reset, tag_counts, tagged  # noqa: E402  (torch first)

import base64_model as B6  # noqa: E402
from multithreading_string_matching_amd.matcher import OPT_NONTEMPORAL, GpuMatcher  # noqa: E402
from test_gpu_base64 import blob, check_arena, plain  # noqa: E402
from test_gpu_decode_scale import tiled  # noqa: E402
from test_gpu_high_destinations import REST, Destination, check_index_and_bytes, check_tags, host_can_hold, periods_above, source  # noqa: E402,F401

MIN_RUN = 16
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


def period(kind, urlsafe=False):
    """257 distinct payloads: a third without a run of 16, the others with base64 blobs -- also across unit and step boundaries --, with and
    without their '='; the last bytes of some a run that ends with the payload"""
    rng = np.random.default_rng(71 if kind == "small" else 72)
    out, seen = [], set()
    while len(out) < PERIOD:
        k = len(out)
        L = int(rng.integers(16, 49)) if kind == "small" else int(rng.integers(2900, 3101))
        t = bytearray(plain(rng, L))
        if k % 3:
            for _ in range(1 + L // 300):
                b = blob(rng, int(rng.integers(12, 24 if kind == "small" else 200)), urlsafe, pad=bool(rng.integers(0, 2)))[:L]
                i = int(rng.integers(0, L - len(b) + 1))
                t[i:i + len(b)] = b
            if k % 5 == 0:
                t[L - 15:] = blob(rng, 12, urlsafe)[:15]
        t = bytes(t)
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def expectation(base, n, urlsafe, only_changed):
    m = B6.load_base64(base, MIN_RUN, urlsafe, only_changed)
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
def periodic(request, src):
    kind = request.param
    base = period(kind)
    n = N_SMALL if kind == "small" else N_LARGE
    per = B6.packed_image(base)
    reps, rest = divmod(n, PERIOD)
    arena, _, ln = tiled(per, reps, rest)
    slot = np.maximum(np.uint64(16), (ln.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15))
    reset(src)
    src.load_arena(np.concatenate([arena, np.zeros(64, np.uint8)]), (np.cumsum(slot) - slot).astype(np.uint64), ln)
    assert src.arena_info() == (n, int(ln.sum(dtype=np.uint64)))
    return base, n


@pytest.mark.parametrize("urlsafe, only_changed", [(False, False), (True, True)])
def test_at_scale(src, dst, periodic, urlsafe, only_changed):
    base, n = periodic
    want = expectation(base, n, urlsafe, only_changed)
    assert 0 < want["stats"]["n_changed"] < n
    try:
        reset(dst)
        res = dst.load_base64(src, min_run=MIN_RUN, urlsafe=urlsafe, only_changed=only_changed)
        assert np.array_equal(res["changed"], want["changed"]) and np.array_equal(res["index"], want["index"])
        assert res["stats"] == want["stats"]
        check_arena(dst, want)
        assert dst.last_timing().launches == 5
    finally:
        reset(dst)


def decoded(base, n, urlsafe, only_changed):
    """what kmpgpu_load_base64 leaves and hands out over the periodic source of n payloads: one period by expectation
    (tests/base64_model.py), the others by index arithmetic"""
    one = expectation(base, PERIOD, urlsafe, only_changed)
    want = periodic_dst((one["arena"], one["off"], one["len"]), one["index"], n)
    reps, rest = divmod(n, PERIOD)
    src_len = np.array([len(t) for t in base], dtype=np.int64)
    want["changed"] = np.concatenate([np.tile(one["changed"], reps), one["changed"][:rest]])
    want["stats"] = {"n_payloads": len(want["len"]), "n_changed": int(want["changed"].sum()),
                     "bytes_in": int(src_len[want["index"] % PERIOD].sum()), "bytes_out": int(want["len"].sum(dtype=np.uint64))}
    out = [B6.decode(base[int(e)], MIN_RUN, urlsafe) for e in one["index"]]
    want["tags"] = tag_counts(out, reps + (one["index"] < rest))
    return want


def test_base64_past_2_32(source):
    """kmpgpu_load_base64 with destinations of 4.45 GB: everything, and the changed payloads alone (a longer source); the straight copy
    (the third of the period without a run) and the staged path both write behind 2^32"""
    base = [tagged(t, e) for e, t in enumerate(period("large"))]
    assert all(B6.decode(t, MIN_RUN).startswith(t[:8]) for t in base)                  # the tags survive
    modes = []
    for urlsafe, only_changed, nontemporal in ((False, False, 1), (False, True, 0)):
        one = expectation(base, PERIOD, urlsafe, only_changed)
        n = periods_above(len(one["arena"]), more=1) * PERIOD + REST
        want = decoded(base, n, urlsafe, only_changed)
        first = -(-B32 // len(want["per"]))                                        # the first full period behind 2^32 is not the last one
        assert first < want["reps"]
        assert want["stats"]["bytes_in"] > B32 and want["stats"]["bytes_out"] > B32 and 0 < want["stats"]["n_changed"] < n
        modes.append((urlsafe, only_changed, nontemporal, n, want))
    host_can_hold(max(m[4]["end"] for m in modes) + 64)
    source.build(base, max(m[3] for m in modes))
    with Destination() as dst:
        for urlsafe, only_changed, nontemporal, n, want in modes:
            src = source.use(n)
            dst.set_option(OPT_NONTEMPORAL, nontemporal)
            res = dst.load_base64(src, min_run=MIN_RUN, urlsafe=urlsafe, only_changed=only_changed)
            assert np.array_equal(res["changed"], want["changed"]) and np.array_equal(res["index"], want["index"])
            assert res["stats"] == want["stats"]
            check_index_and_bytes(dst, want)
            check_tags(dst, want["tags"])
    source.release()
