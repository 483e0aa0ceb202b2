"""The host code kmpgpu_load_tls adds -- the parser of KMPGPU_TLS_FIELD's value (csrc/host/kmp_cli_tls.h) -- as a stand-alone program
under AddressSanitizer + UBSan (tests/tls_sanitizer_driver.c).  No GPU needed."""
import os
import shutil
import subprocess

import pytest


def test_tls_value_parser_under_sanitizers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tls_driver")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(root, "multithreading_string_matching_amd", "csrc", "host"),
           os.path.join(root, "tests", "tls_sanitizer_driver.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "tls driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
