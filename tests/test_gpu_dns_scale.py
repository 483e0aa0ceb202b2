"""kmpgpu_dns_locate / kmpgpu_load_dns past every grid cap of csrc/kmp_dns.hip, on a real MI355X.

  kmp_dns_locate_kernel     DNS_LOCATE_BLOCKS 2 048 blocks * 4 wavefronts * 64 payloads: a second round past 524 288 payloads
  kmp_dns_lengths_kernel    kmp_group_blocks: KMP_GRID_CAP 1 024 * 4 * 64, past 262 144 payloads
  kmp_dns_index_kernel      kmp_item_blocks: KMP_GRID_CAP 1 024 * 256 threads, past 262 144 payloads
  kmp_scan_totals_kernel    one round of 256 block totals (kmp_prep.hip)
  kmp_dns_gather_kernel     KMP_GRID_CAP 1 024 * 4 runs: past 4 096 runs of 64 names

The arena is periodic (gpu_support.PeriodicSource): 257 distinct payloads -- no messages, root questions, short names and names of 255
bytes on the wire --, repeated, laid out on the device.  tests/dns_model.py locates the 257 once; what the spans and dst have to hold
-- index, lengths, offsets, every byte -- follows from the period by index arithmetic (gpu_support.periodic_dst), and is compared
exactly.

Run on a real MI355X:  python -m pytest tests/test_gpu_dns_scale.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import PERIOD, PeriodicSource, check_periodic_bytes, periodic_dst, reset  # noqa: E402  (torch first)

import dns_model as DNS  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

N = 600_001
assert N > 2048 * 4 * 64


def period():
    """257 distinct payloads"""
    rng = np.random.default_rng(73)
    out = []
    for k in range(PERIOD):
        tag = b"%03d" % k
        kind = k % 5
        if kind == 0:
            t = b"no dns " + tag + b"\xff" * int(rng.integers(0, 40))
        elif kind == 1:
            t = DNS.message([], ident=k, tail=tag)                                     # the root name
        elif kind == 2:
            t = DNS.message([tag, b"x" * 57, b"y" * 63, b"z" * 63, b"w" * 63], ident=k, flags=0x8180)          # 255 bytes on the wire
        elif kind == 3:
            t = DNS.message([tag], ident=k)[:-5] + b"\xc0\x0c\x00\x01\x00\x01"                          # a pointer behind a label
        else:
            t = DNS.message([tag] + [rng.integers(0x61, 0x7B, int(rng.integers(1, 12)), dtype=np.uint8).tobytes() for _ in range(k % 4)],
                            ident=k, flags=0x8180 if k % 2 else 0x0100, tail=bytes(int(rng.integers(0, 30))))
        out.append(t)
    assert len(set(out)) == PERIOD
    return out


def gather_runs(n_dst, total_bytes):
    """the runs kmp_launch_dns_gather cuts dst into: what brings an average run to 16 KiB, a power of two up to 64 payloads"""
    avg, run = max(total_bytes // n_dst, 16), 64
    while run > 1 and run * avg > 16384:
        run >>= 1
    return run, -(-n_dst // run)


def expectation(base, n, only_present):
    one = DNS.load_dns(base, only_present)
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
    kinds = DNS.spans(base)["kind"]
    lens = DNS.spans(base)["name_len"]
    assert (kinds == DNS.NONE).sum() > 100 and (kinds == DNS.QUERY).sum() > 50 and (kinds == DNS.RESPONSE).sum() > 50 and lens.max() == 253
    reps, rest = divmod(N, PERIOD)
    times = reps + (np.arange(PERIOD) < rest)
    try:
        reset(dst)
        src = source.build(base, N)
        # the locate: every record, and the totals
        per_entry = [DNS.locate_stats([t]) for t in base]
        assert src.dns_locate() == {f: int(sum(int(x) * s[f] for x, s in zip(times, per_entry))) for f in per_entry[0]}
        one = DNS.spans(base)
        got = src.dns_spans()
        assert got[:reps * PERIOD].tobytes() == np.tile(one, reps).tobytes() and got[reps * PERIOD:].tobytes() == one[:rest].tobytes()
        for only_present in (True, False):
            want = expectation(base, N, only_present)
            assert 0 < want["stats"]["n_present"] < N
            run, n_runs = gather_runs(len(want["len"]), want["end"])
            assert run == 64 and n_runs > 4096 and len(want["len"]) > 1024 * 4 * 64
            res = dst.load_dns(src, only_present=only_present)
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
