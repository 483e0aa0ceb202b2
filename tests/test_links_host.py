"""The rules' table with the links' rows behind the expressions' (csrc/kmp_rowtables.cpp, the kmp_pack_rules entry that takes n_links):
packed and checked on the host, so tested here without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")


def test_rules_over_links_pack_under_sanitizers(tmp_path):
    """plain g++ under ASan + UBSan, driven by tests/links_sanitizer_driver.cpp (a program of its own) against tables written out by hand"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "links_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, os.path.join(ROOT, "tests", "links_sanitizer_driver.cpp"), os.path.join(CSRC, "kmp_rowtables.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "links driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_links_and_rules_file_parsers_under_sanitizers(tmp_path):
    """csrc/host/kmphost.c (kmp_links_parse, kmp_rules_parse_links) and csrc/host/kmp_cli_links.h with plain gcc under ASan + UBSan,
    driven by tests/links_parsers_sanitizer_driver.c, a program of its own"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "links_parsers_driver")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(CSRC, "host"),
           os.path.join(ROOT, "tests", "links_parsers_sanitizer_driver.c"), os.path.join(CSRC, "host", "kmphost.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "links parsers driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_link_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_links.hip" in hipsrc.split()
