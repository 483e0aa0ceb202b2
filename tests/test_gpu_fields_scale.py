"""kmpgpu_http_locate / kmpgpu_load_fields past every grid cap of csrc/kmp_fields.hip, on a real MI355X.

  kmp_http_locate_kernel      FLD_LOCATE_BLOCKS 2 048 blocks * 4 wavefronts * 64 payloads: a second round past 524 288 payloads; payloads of
                              ~3 000 bytes take three steps of 1 KiB each
  kmp_fields_lengths_kernel   KMP_GRID_CAP 1 024 * 4 * 64: past 262 144 payloads
  kmp_fields_index_kernel     KMP_GRID_CAP 1 024 * 256 threads: past 262 144 payloads
  kmp_scan_totals_kernel      one round of 256 block totals (kmp_prep.hip)
  kmp_fields_gather_kernel    KMP_GRID_CAP 1 024 * 4 runs: past 4 096 runs -- runs of 64 fields of 0..40 bytes (262 144 payloads), runs
                              of 4 fields of ~2 600 bytes (16 384 payloads of dst)

The arenas are periodic (gpu_support.PeriodicSource): 257 distinct payloads, repeated, laid out on the device.  tests/http_model.py
locates the 257 once; what the spans and dst have to hold -- index, lengths, offsets, every byte -- follows from the period by index
arithmetic (gpu_support.periodic_dst), and is compared exactly.

Run on a real MI355X:  python -m pytest tests/test_gpu_fields_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import PERIOD, PeriodicSource, check_periodic_bytes, periodic_dst, reset  # noqa: E402  (torch first)

import http_model as HM  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

N_SMALL, N_LARGE = 600_001, 26_001
assert N_SMALL > 2048 * 4 * 64 and N_LARGE * 2 // 3 > 1024 * 4 * 4
CASES = {"small": (N_SMALL, [("raw_uri", False), ("status", True)]), "large": (N_LARGE, [("body", True), ("headers", False)])}          # the first case of each passes the gather's cap


def filler(rng, L):
    return rng.choice(np.frombuffer(b"abcXYZ019/%=&.-", dtype=np.uint8), L).tobytes()


def period(kind):
    """257 distinct payloads: requests, responses, messages without a blank line and other traffic"""
    rng = np.random.default_rng(71 if kind == "small" else 72)
    out, seen = [], set()
    while len(out) < PERIOD:
        k = len(out)
        nl = b"\r\n" if k % 2 else b"\n"
        if kind == "small":
            t = [b"GET /" + filler(rng, int(rng.integers(0, 36))) + b" H" + nl + nl + filler(rng, int(rng.integers(0, 8))),
                 b"HTTP/1.1 %d" % (100 + k) + b" OK" + nl, filler(rng, int(rng.integers(0, 48))), b"POST /" + filler(rng, int(rng.integers(0, 30)))][k % 4]
        else:
            hdr = b"Host: " + filler(rng, int(rng.integers(20, 1200))) + nl
            rest = filler(rng, int(rng.integers(2800, 3000)) - len(hdr))
            t = [b"POST /" + filler(rng, k % 23) + b" HTTP/1.1" + nl + hdr + nl + rest, b"HTTP/1.1 200 OK" + nl + hdr + rest,
                 b"GET /" + filler(rng, k % 19) + nl + nl + rest + hdr][k % 3]
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def gather_runs(n_dst, total_bytes):
    """the runs kmp_launch_fields_gather cuts dst into: what brings an average run to 16 KiB, a power of two up to 64 payloads"""
    avg, run = max(total_bytes // n_dst, 16), 64
    while run > 1 and run * avg > 16384:
        run >>= 1
    return run, -(-n_dst // run)


def expectation(base, n, field, only_present):
    one = HM.load_fields(base, field, only_present)
    want = periodic_dst((one["arena"], one["off"].astype(np.int64), one["len"].astype(np.int64)), one["index"], n)
    reps, rest = divmod(n, PERIOD)
    src_len = np.array([len(t) for t in base], dtype=np.int64)
    want["present"] = np.concatenate([np.tile(one["present"], reps), one["present"][:rest]])
    want["stats"] = {"n_payloads": len(want["len"]), "n_present": int(want["present"].sum()),
                     "bytes_in": int(src_len[want["index"] % PERIOD].sum()), "bytes_out": int(want["len"].sum(dtype=np.uint64))}
    return want


@pytest.fixture(scope="module")
def source():
    s = PeriodicSource()
    yield s
    s.close()


@pytest.fixture(scope="module")
def dst():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.mark.parametrize("kind", ["small", "large"])
def test_at_scale(source, dst, kind):
    n, cases = CASES[kind]
    base = period(kind)
    reps, rest = divmod(n, PERIOD)
    times = reps + (np.arange(PERIOD) < rest)
    try:
        reset(dst)
        src = source.build(base, n)
        # the locate: every record, and the totals
        per_entry = [HM.locate_stats([t]) for t in base]
        assert src.http_locate() == {f: int(sum(int(x) * s[f] for x, s in zip(times, per_entry))) for f in per_entry[0]}
        one = HM.spans(base)
        got = src.http_spans()
        assert got[:reps * PERIOD].tobytes() == np.tile(one, reps).tobytes() and got[reps * PERIOD:].tobytes() == one[:rest].tobytes()
        if kind == "large":
            assert min(len(t) for t in base) > 2048                                # three steps each
        for field, only_present in cases:
            want = expectation(base, n, field, only_present)
            assert 0 < want["stats"]["n_present"] <= n
            if (field, only_present) == cases[0]:
                run, n_runs = gather_runs(len(want["len"]), want["end"])
                assert want["stats"]["n_present"] < n and run == (64 if kind == "small" else 4) and n_runs > 4096
            res = dst.load_fields(src, field=field, only_present=only_present)
            assert np.array_equal(res["present"], want["present"]) and np.array_equal(res["index"], want["index"])
            assert res["stats"] == want["stats"]
            assert dst.arena_info() == (len(want["len"]), int(want["len"].sum(dtype=np.uint64)))
            a, off, ln = dst.arena_download()
            assert np.array_equal(off, want["off"]) and np.array_equal(ln, want["len"])
            check_periodic_bytes(a, want)
            assert dst.last_timing().launches == 5
    finally:
        reset(dst)
        source.release()
