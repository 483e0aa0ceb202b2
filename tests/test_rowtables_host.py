"""The tables of the rules, windows, relations and chains as the kernels read them (csrc/kmp_rowtables.cpp): packed and checked on the
host, so tested here without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")


def test_row_table_packers_under_sanitizers(tmp_path):
    """csrc/kmp_rowtables.cpp (host code without a HIP header) with plain g++ under ASan + UBSan, driven by
    tests/rowtables_sanitizer_driver.cpp against tables written out by hand."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rowtables_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, os.path.join(ROOT, "tests", "rowtables_sanitizer_driver.cpp"), os.path.join(CSRC, "kmp_rowtables.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "rowtables driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_packers_are_in_the_build_and_take_no_hip_header():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_rowtables.cpp" in hipsrc.split()
    for name in ("kmp_rowtables.cpp", "kmp_rowtables.h"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip/" not in f.read()
