"""The rate thresholds' host side without a GPU: the packer of their tables (csrc/kmp_rowtables.cpp: kmp_pack_thresholds), the parser of
their file (csrc/host/kmphost.c: kmp_thresholds_parse) and the reader of a capture's timestamps (kmp_arena_from_pcap_ts) under ASan +
UBSan in a stand-alone program, tests/thresholds_sanitizer_driver.cpp; and the Python layer's view of the same."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import DATA

from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.host import HostArena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")


def test_threshold_packer_parser_and_timestamps_under_sanitizers(tmp_path):
    """every refusal of the packer and a hand-made table; the file parser's refusals line by line and its exact microseconds; the
    timestamps of classic captures in both byte orders, under the nanosecond magic, of a pcapng section and of tests/golden/data/tcp.pcap"""
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no gcc / g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    host_o, exe = str(tmp_path / "kmphost.o"), str(tmp_path / "thresholds_driver")
    subprocess.run(["gcc", "-std=gnu11", "-fopenmp", *san, *inc, "-c", os.path.join(CSRC, "host", "kmphost.c"), "-o", host_o],
                   check=True, capture_output=True, timeout=300)
    subprocess.run(["g++", "-std=c++17", "-fopenmp", *san, *inc, os.path.join(ROOT, "tests", "thresholds_sanitizer_driver.cpp"),
                    os.path.join(CSRC, "kmp_rowtables.cpp"), host_o, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path), os.path.join(DATA, "tcp.pcap")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "thresholds driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_the_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_thresholds.hip" in hipsrc.split()


def test_constants_match_the_headers():
    with open(os.path.join(ROOT, "include", "kmpgpu.h")) as f:
        text = f.read()
    for name, value in _lib.THR_TRACKS.items():
        assert f"#define KMPGPU_THR_{name.upper():<8} {value}\n" in text, name
    for name, value in _lib.THR_TYPES.items():
        assert f"#define KMPGPU_THR_{name.upper():<8} {value}\n" in text, name
    assert "#define KMPGPU_THR_NO_WINDOW (~0ull)\n" in text and _lib.THR_NO_WINDOW == 2 ** 64 - 1
    assert ctypes.sizeof(_lib.Threshold) == 24


def test_the_parser_through_the_host_library(tmp_path):
    """kmp_thresholds_parse as libkmphost.so exports it: the thresholds and a refusal"""
    H = _lib.host_lib()
    path = tmp_path / "thresholds.txt"
    path.write_text("# the fifth failed login from one address within a minute; one alert per source and minute\n0 by_src at_least 5 60\n1 by_src at_most 1 60\n"
                    "1 by_rule exactly 3 all\n0 by_flow at_least 2 0.25\n")
    f, err = _lib.Thresholds(), ctypes.create_string_buffer(256)
    assert H.kmp_thresholds_parse(str(path).encode(), 2, ctypes.byref(f), err) == 0 and err.value == b""
    assert f.n == 4
    assert [(f.thr[i].rule, f.thr[i].track, f.thr[i].type, f.thr[i].count, f.thr[i].window) for i in range(4)] == \
        [(0, 1, 0, 5, 60_000_000), (1, 1, 1, 1, 60_000_000), (1, 0, 2, 3, 2 ** 64 - 1), (0, 3, 0, 2, 250_000)]
    H.kmp_thresholds_free(ctypes.byref(f))
    assert f.n == 0 and not f.thr
    assert H.kmp_thresholds_parse(str(path).encode(), 1, ctypes.byref(f), err) != 0 and err.value == b"line 3: rule 1 of 1"
    H.kmp_thresholds_free(ctypes.byref(f))


def test_from_pcap_with_ts():
    """HostArena.from_pcap(with_ts=True): the records' ts_sec * 1e6 + ts_usec, read here from the file, for the frames the extractor
    accepts; the arena and the metadata are what they are without"""
    for name, proto in (("tcp.pcap", "tcp"), ("udp.pcap", "udp")):
        path = os.path.join(DATA, name)
        b = open(path, "rb").read()
        assert b[:4] == bytes.fromhex("d4c3b2a1")
        times, pos = [], 24
        while pos + 16 <= len(b):
            sec, usec, caplen, _ = struct.unpack_from("<IIII", b, pos)
            times.append(sec * 1_000_000 + usec)
            pos += 16 + caplen
        plain = HostArena.from_pcap(path, proto, with_meta=True, with_seq=True)
        for with_meta, with_seq in ((False, False), (True, False), (True, True)):
            a = HostArena.from_pcap(path, proto, with_meta=with_meta, with_seq=with_seq, with_ts=True)
            assert a.ts.dtype == np.uint64 and a.n_pkts == plain.n_pkts == len(a.ts) and a.n_frames == len(times)
            if a.n_pkts == a.n_frames:
                assert a.ts.tolist() == times
            assert set(a.ts.tolist()) <= set(times) and (np.diff(a.ts.astype(np.int64)) >= 0).all()
            assert np.array_equal(a.bytes, plain.bytes) and np.array_equal(a.off, plain.off) and np.array_equal(a.len, plain.len)
            assert (a.meta is None) == (not with_meta) and (a.meta is None or np.array_equal(a.meta, plain.meta))
            assert (a.seq is None) == (not with_seq) and (a.seq is None or np.array_equal(a.seq, plain.seq))
        assert HostArena.from_pcap(path, proto).ts is None
    assert HostArena.from_pcap(os.path.join(DATA, "tcp.pcap"), "tcp", with_ts=True).n_pkts == 13
