"""tests/scan_matrix.py against what the compiler emits for the three scan files (no GPU needed: hipcc cross-compiles gfx950).

Only symbol names are read: the `.amdhsa_kernel` lines of the device assembly, demangled by c++filt.  A launcher that gains an
instantiation fails here until scan_matrix.py has a row for it (or names it UNREACHABLE, with the line that makes it so); a row that
is deleted, or names a kernel that no longer exists, fails here too."""
import os
import re
import shutil
import subprocess

import pytest

import scan_matrix as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emitted(tmp_path_factory):
    """{source: the normalised names of its kernels}"""
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not os.path.exists(HIPCC) or not cxxfilt:
        pytest.skip("hipcc or c++filt not installed")
    tmp = str(tmp_path_factory.mktemp("names"))
    # -O1: the names do not depend on the level, and -O0 does not get through the kernels' inline assembly; the three files side by side
    procs = {src: subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1048576",
                                    f"-I{ROOT}/include", f"-I{CSRC}", "-S", "--cuda-device-only", "-o", os.path.join(tmp, src + ".s"),
                                    os.path.join(CSRC, src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for src in SM.SOURCES}
    out = {}
    for src, p in procs.items():
        log, _ = p.communicate(timeout=900)
        assert p.returncode == 0, log[-3000:]
        with open(os.path.join(tmp, src + ".s")) as f:
            mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), re.M)
        assert mangled, src
        r = subprocess.run([cxxfilt], input="\n".join(mangled) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        names = [SM.normalise(line) for line in r.stdout.splitlines()]
        assert len(names) == len(mangled) == len(set(names)), src
        out[src] = names
    return out


def test_the_table_is_what_the_compiler_emitted(emitted):
    got = {n for names in emitted.values() for n in names if SM.is_scan_kernel(n)}
    rows = {r["name"] for r in SM.ROWS}
    missing = sorted(got - rows - set(SM.UNREACHABLE))
    surplus = sorted((rows | set(SM.UNREACHABLE)) - got)
    assert not missing, "instantiations without a row in tests/scan_matrix.py (add a row that launches each, or name it UNREACHABLE): %s" % missing
    assert not surplus, "tests/scan_matrix.py names instantiations that the compiler no longer emits: %s" % surplus
    # every other kernel of the three files is one the table does not claim: the bitmap and plan builders
    assert sorted({n for names in emitted.values() for n in names} - got) == ["kmp_build_bitmap_kernel", "kmp_plan_kernel"]
    per_file = {src: sum(1 for n in names if SM.is_scan_kernel(n)) for src, names in emitted.items()}
    print(per_file, len(rows), len(SM.UNREACHABLE))
    assert per_file == {"kmp_scan_stream.hip": 26, "kmp_scan_general.hip": 36, "kmp_scan_multi.hip": 56}


def test_rows_and_unreachable_are_disjoint_and_no_row_twice():
    names = [r["name"] for r in SM.ROWS]
    twice = sorted({n for n in names if names.count(n) > 1})
    assert not twice, twice
    both = sorted(set(names) & set(SM.UNREACHABLE))
    assert not both, both
    assert SM.BY_NAME.keys() == set(names)
    for name, why in SM.UNREACHABLE.items():
        assert SM.is_scan_kernel(name) and "KMP_MULTI_LAUNCH" in why, name
    # the launcher lines the reasons quote are lines of the launcher
    with open(os.path.join(CSRC, "kmp_scan_multi.hip")) as f:
        text = f.read()
    for why in set(SM.UNREACHABLE.values()):
        for quoted in re.findall(r"`([^`]+)`", why):
            if "..." not in quoted and ".." not in quoted:
                assert quoted in text, quoted


def test_rows_are_well_formed():
    names = {r["name"] for r in SM.ROWS}
    for r in SM.ROWS:
        assert SM.is_scan_kernel(r["name"]) and SM.normalise(r["name"]) == r["name"], r["name"]
        assert r["arena"] in SM.ARENAS and r["patterns"] in SM.PATTERNS and r["call"] in SM.CALLS, r
        assert r["family"] in ("flat", "packed", "general", "fused"), r
        # what a row launches besides has a row of its own
        assert all(a in names and a != r["name"] for a in r["also"]), r
        # the flat kernel needs a uniform arena, and only it is given one
        assert (r["family"] == "flat") == r["arena"].startswith("uniform"), r
        # a pass that emits takes no general kernel
        assert r["call"] == "scan" or r["family"] != "general", r
        assert ("emit_kernel<" in r["name"] or r["name"].endswith(", true, true>") and r["family"] in ("flat", "packed")) == (r["call"] != "scan"), r


def test_every_option_value_is_one_the_library_accepts():
    with open(os.path.join(CSRC, "kmpgpu.hip")) as f:
        text = f.read()
    for msg in SM.REFUSALS:                                 # the rules ACCEPTED was written from are still the library's
        assert msg in text, msg
    with open(os.path.join(ROOT, "include", "kmpgpu.h")) as f:
        header = f.read()
    for key, number in SM.OPTIONS.items():
        assert re.search(r"^#define KMPGPU_OPT_%s\s+%d\b" % (key, number), header, re.M), key
    for r in SM.ROWS:
        for key, value in r["options"].items():
            assert key in SM.OPTIONS and value in SM.ACCEPTED[key], (r["name"], key, value)
