"""The flow bits' host side without a GPU: the packer of their tables (csrc/kmp_rowtables.cpp: kmp_pack_flowbits) and the parser of their
file (csrc/host/kmphost.c: kmp_flowbits_parse) under ASan + UBSan in a stand-alone program, tests/flowbits_sanitizer_driver.cpp; and the
Python layer's own checks."""
import ctypes
import os
import shutil
import subprocess

import pytest

from multithreading_string_matching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")


def test_flowbit_packer_and_parser_under_sanitizers(tmp_path):
    """every refusal of the packer, the levels and records of hand-made graphs, cycles of length 2 and 3, a self-loop accepted, and the
    file parser's refusals line by line"""
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no gcc / g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    host_o, exe = str(tmp_path / "kmphost.o"), str(tmp_path / "flowbits_driver")
    subprocess.run(["gcc", "-std=gnu11", "-fopenmp", *san, *inc, "-c", os.path.join(CSRC, "host", "kmphost.c"), "-o", host_o],
                   check=True, capture_output=True, timeout=300)
    subprocess.run(["g++", "-std=c++17", "-fopenmp", *san, *inc, os.path.join(ROOT, "tests", "flowbits_sanitizer_driver.cpp"),
                    os.path.join(CSRC, "kmp_rowtables.cpp"), host_o, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "flowbits driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_the_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_flowbits.hip" in hipsrc.split()


def test_constants_match_the_headers():
    with open(os.path.join(ROOT, "include", "kmpgpu.h")) as f:
        text = f.read()
    assert f"#define KMPGPU_FLOWBITS_MAX {_lib.FLOWBITS_MAX}\n" in text
    for name, value in _lib.FLOWBIT_OPS.items():
        assert f"#define KMPGPU_FB_{name.upper():<8} {value}\n" in text, name
    assert ctypes.sizeof(_lib.FlowbitOp) == 16


def test_the_parser_through_the_host_library(tmp_path):
    """kmp_flowbits_parse as libkmphost.so exports it: the ops, the names and a refusal"""
    H = _lib.host_lib()
    path = tmp_path / "flowbits.txt"
    path.write_text("# once per connection\n0 isnotset:seen set:seen\n1 isset:seen noalert\n")
    f, err = _lib.Flowbits(), ctypes.create_string_buffer(256)
    assert H.kmp_flowbits_parse(str(path).encode(), 2, ctypes.byref(f), err) == 0 and err.value == b""
    assert (f.n, f.n_bits, f.names[0].value) == (4, 1, b"seen")
    assert [(f.ops[i].rule, f.ops[i].bit, f.ops[i].op, f.ops[i].reserved) for i in range(4)] == [(0, 0, 1, 0), (0, 0, 2, 0), (1, 0, 0, 0), (1, 0, 5, 0)]
    H.kmp_flowbits_free(ctypes.byref(f))
    assert f.n == 0 and not f.ops
    assert H.kmp_flowbits_parse(str(path).encode(), 1, ctypes.byref(f), err) != 0 and err.value == b"line 3: rule 1 of 1"
    H.kmp_flowbits_free(ctypes.byref(f))
