"""kmpgpu_tls_locate / kmpgpu_load_tls past every grid cap of csrc/kmp_tls.hip, on a real MI355X.

  kmp_tls_locate_kernel     TLS_LOCATE_BLOCKS 2 048 blocks * 4 wavefronts * 64 payloads: a second round past 524 288 payloads
  kmp_tls_lengths_kernel    kmp_group_blocks: KMP_GRID_CAP 1 024 * 4 * 64, past 262 144 payloads
  kmp_tls_index_kernel      kmp_item_blocks: KMP_GRID_CAP 1 024 * 256 threads, past 262 144 payloads
  kmp_scan_totals_kernel    one round of 256 block totals (kmp_prep.hip)
  kmp_tls_gather_kernel     KMP_GRID_CAP 1 024 * 4 runs: past 4 096 runs of 64 fields

The arena is periodic (gpu_support.PeriodicSource): 257 distinct payloads -- short hellos with both fields, with one, with none,
malformed ones and payloads that are no hello --, repeated, laid out on the device.  tests/tls_model.py locates the 257 once; what the
spans and dst have to hold -- index, lengths, offsets, every byte -- follows from the period by index arithmetic
(gpu_support.periodic_dst), and is compared exactly.

Run on a real MI355X:  python -m pytest tests/test_gpu_tls_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import PERIOD, PeriodicSource, check_periodic_bytes, periodic_dst, reset  # noqa: E402  (torch first)

import tls_model as TLS  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

N = 600_001
assert N > 2048 * 4 * 64
H, SNI, ALPN, EXT = TLS.hello, TLS.sni_ext, TLS.alpn_ext, TLS.ext


def period():
    """257 distinct payloads"""
    rng = np.random.default_rng(173)
    out = []
    for k in range(PERIOD):
        tag = b"%03d" % k
        kind = k % 5
        if kind == 0:
            t = b"no tls " + tag + b"\xff" * int(rng.integers(0, 40))
        elif kind == 1:
            t = H([SNI(tag + b".example.com"), ALPN([b"h2", b"http/1.1"])], sid=k % 33, suites=1 + k % 4)
        elif kind == 2:
            t = H([ALPN([tag] + [b"p%d" % i for i in range(k % 30)]), SNI(tag + b"." + b"x" * (k % 61))], sid=0, suites=1)
        elif kind == 3:
            t = H([EXT(100 + i, bytes(i)) for i in range(k % 6)] + [SNI(tag), EXT(21, bytes(k % 40)), ALPN([b"h3", tag])], sid=k % 33, suites=2)
        elif k % 2:
            t = H([SNI(tag + b".example.org", nl=17)], sid=0, suites=1)                 # a name that leaves its list
        else:
            t = H([SNI(tag + b".sni-only.example")], sid=8, suites=1)[:-(k % 3)or None]
        out.append(t)
    assert len(set(out)) == PERIOD
    return out


def gather_runs(n_dst, total_bytes):
    """the runs kmp_launch_tls_gather cuts dst into: what brings an average run to 16 KiB, a power of two up to 64 payloads"""
    avg, run = max(total_bytes // n_dst, 16), 64
    while run > 1 and run * avg > 16384:
        run >>= 1
    return run, -(-n_dst // run)


def expectation(base, n, field, only_present):
    one = TLS.load_tls(base, field, only_present)
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


def test_at_scale(source, dst):
    base = period()
    one = TLS.spans(base)
    assert (one["kind"] == TLS.NONE).sum() > 70 and (one["flags"] & TLS.HAS_SNI != 0).sum() > 150 and (one["flags"] & TLS.HAS_ALPN != 0).sum() > 150
    assert (one["flags"] & TLS.TRUNCATED != 0).sum() > 10 and one["alpn_len"].max() > 100
    reps, rest = divmod(N, PERIOD)
    times = reps + (np.arange(PERIOD) < rest)
    try:
        reset(dst)
        src = source.build(base, N)
        # the locate: every record, and the totals
        per_entry = [TLS.locate_stats([t]) for t in base]
        assert src.tls_locate() == {f: int(sum(int(x) * s[f] for x, s in zip(times, per_entry))) for f in per_entry[0]}
        got = src.tls_spans()
        assert got[:reps * PERIOD].tobytes() == np.tile(one, reps).tobytes() and got[reps * PERIOD:].tobytes() == one[:rest].tobytes()
        for field, only_present in (("sni", True), ("alpn", True), ("alpn", False)):
            want = expectation(base, N, field, only_present)
            assert 0 < want["stats"]["n_present"] < N
            run, n_runs = gather_runs(len(want["len"]), want["end"])
            assert run == 64 and n_runs > 4096 and len(want["len"]) > 1024 * 4 * 64
            res = dst.load_tls(src, field=field, only_present=only_present)
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
