"""The host side of the byte tests (include/kmphost.h: kmp_bytetests_parse, kmp_rules_parse_bt) and the packers of csrc/kmp_rowtables.cpp
(kmp_pack_bytetests and the n_bt entries of its siblings) under sanitizers: no GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bytetest_model as BM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.host import BYTETEST_DTYPE, parse_bytetests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")
NOT = _lib.RULE_NOT
EIO, EINVAL = -1, -4                                   # KMPHOST_EIO, KMPHOST_EINVAL
U32 = 0xFFFFFFFF


def test_layouts_and_constants():
    assert BYTETEST_DTYPE.itemsize == C.sizeof(_lib.ByteTest) == 20
    for name in BYTETEST_DTYPE.names:
        assert BYTETEST_DTYPE.fields[name][1] == getattr(_lib.ByteTest, name).offset, name
    assert (_lib.BT_RELATIVE, _lib.BT_LITTLE) == (BM.RELATIVE, BM.LITTLE) == (1, 2)
    assert (_lib.BT_EQ, _lib.BT_NE, _lib.BT_LT, _lib.BT_GT, _lib.BT_LE, _lib.BT_GE) == (BM.EQ, BM.NE, BM.LT, BM.GT, BM.LE, BM.GE)
    # the constants of the two headers and of the launch header
    for header, prefix in (("kmpgpu.h", "KMPGPU_BT"), ("kmphost.h", "KMP_BT")):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert f"#define {prefix}_RELATIVE" in text and f"enum {{ {prefix}_EQ, {prefix}_NE, {prefix}_LT, {prefix}_GT, {prefix}_LE, {prefix}_GE }};" in text
    assert f"#define KMP_BT_TILE {_lib.BT_TILE}u" in open(os.path.join(CSRC, "kmp_launch.h")).read()


# ------------------------------------------------------------------------------------------------
# the byte tests file
# ------------------------------------------------------------------------------------------------
def _tests(tmp_path, text, n_pat=3):
    path = tmp_path / "bytetests.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    b = _lib.ByteTests()
    err = C.create_string_buffer(_lib.KMP_BYTETESTS_ERRBUF)
    rc = L.kmp_bytetests_parse(str(path).encode(), n_pat, C.byref(b), err)
    if rc:
        assert b.n == 0 and not b.bt
        return rc, None, err.value.decode()
    try:
        return 0, [(t.anchor, t.offset, t.mask, t.value, t.nbytes, t.op, t.flags, t.reserved) for t in (b.bt[i] for i in range(b.n))], err.value.decode()
    finally:
        L.kmp_bytetests_free(C.byref(b))


def test_a_byte_tests_file(tmp_path):
    text = (b"# DNS\n"
            b"2 & 0x8000 2\n"
            b"\n"
            b"  2 = 1 4\r\n"
            b"1 >= 0 11 \n"
            b"2 > 512 0 after 1\n"
            b"4 != 0xdeadBEEF -4 after 0 little mask 0x00ffFF00\n"
            b"3 <= 4294967295 0X10 mask 7 little\n"
            b"1 < 255 2147483647 little after 2\n"
            b"\t4 = 0 -2147483648 after 0\n")
    rc, tests, msg = _tests(tmp_path, text)
    assert rc == 0 and msg == ""
    assert tests == [
        (0, 2, 0x8000, 0, 2, BM.NE, 0, 0),
        (0, 4, U32, 1, 2, BM.EQ, 0, 0),
        (0, 11, U32, 0, 1, BM.GE, 0, 0),
        (1, 0, U32, 512, 2, BM.GT, BM.RELATIVE, 0),
        (0, -4, 0x00FFFF00, 0xDEADBEEF, 4, BM.NE, BM.RELATIVE | BM.LITTLE, 0),
        (0, 16, 7, U32, 3, BM.LE, BM.LITTLE, 0),
        (2, 0x7FFFFFFF, U32, 255, 1, BM.LT, BM.RELATIVE | BM.LITTLE, 0),
        (0, -(1 << 31), U32, 0, 4, BM.EQ, BM.RELATIVE, 0),
    ]
    # the Python view of the same file
    arr = parse_bytetests(str(tmp_path / "bytetests.txt"), 3)
    assert arr.dtype == BYTETEST_DTYPE and [tuple(int(x) for x in r) for r in arr] == tests
    # a file of comments and blank lines holds no test
    assert _tests(tmp_path, b"# nothing\n\n   \n")[1] == []


@pytest.mark.parametrize("text, line, what", [
    (b"2 = 1\n", 1, "3 of the four fields that begin <nbytes> <op> <value> <offset>"),
    (b"# c\n\n2\n", 3, "1 of the four fields"),
    (b"0 = 1 0\n", 1, "'0' is not a byte count (1..4)"),
    (b"5 = 1 0\n", 1, "'5' is not a byte count (1..4)"),
    (b"two = 1 0\n", 1, "'two' is not a byte count (1..4)"),
    (b"2 == 1 0\n", 1, "'==' is not an operator (= != < > <= >= &)"),
    (b"2 ! 1 0\n", 1, "'!' is not an operator"),
    (b"2 = -1 0\n", 1, "'-1' is not a value (0..4294967295, decimal or 0x hex)"),
    (b"2 = 4294967296 0\n", 1, "'4294967296' is not a value"),
    (b"2 = 0x 0\n", 1, "'0x' is not a value"),
    (b"2 = 0x1g 0\n", 1, "'0x1g' is not a value"),
    (b"2 = 1f 0\n", 1, "'1f' is not a value"),
    (b"2 = 1 x\n", 1, "'x' is not an offset"),
    (b"2 = 1 2147483648\n", 1, "'2147483648' is not an offset"),
    (b"2 = 1 -2147483649 after 0\n", 1, "'-2147483649' is not an offset"),
    (b"2 = 1 -1\n", 1, "offset -1 lies in front of the payload: only a test after a pattern reaches back"),
    (b"2 = 1 0 after\n", 1, "'after' without a pattern index"),
    (b"2 = 1 0 after x\n", 1, "'x' is not a pattern index"),
    (b"2 = 1 0 after 3\n", 1, "pattern index 3, but there are 3 patterns"),
    (b"2 = 1 0 after 0 after 1\n", 1, "'after' twice"),
    (b"2 = 1 0 little little\n", 1, "'little' twice"),
    (b"2 = 1 0 mask 1 mask 2\n", 1, "'mask' twice"),
    (b"2 = 1 0 mask\n", 1, "'mask' without a mask"),
    (b"2 = 1 0 mask -1\n", 1, "'-1' is not a mask (0..4294967295, decimal or 0x hex)"),
    (b"2 & 1 0 mask 1\n", 1, "'&' takes its mask from <value>: it has no mask clause"),
    (b"2 = 1 0 big\n", 1, "'big' is none of after <pattern index>, little, mask <m>"),
    (b"2 = 1 0 # no\n", 1, "'#' is none of after"),
    (b"2 = 1 0 after 0 little mask 1 x y z\n", 1, "more fields than"),
    (b"2 = 1 0\n2 = 1 0\n9 = 1 0\n", 3, "'9' is not a byte count"),
])
def test_refused_byte_tests_files(tmp_path, text, line, what):
    rc, tests, msg = _tests(tmp_path, text)
    assert rc == EINVAL and tests is None
    assert msg.startswith(f"line {line}: ") and what in msg, msg


def test_missing_byte_tests_file(tmp_path):
    L = _lib.host_lib()
    b = _lib.ByteTests()
    err = C.create_string_buffer(_lib.KMP_BYTETESTS_ERRBUF)
    assert L.kmp_bytetests_parse(str(tmp_path / "nope.txt").encode(), 3, C.byref(b), err) == EIO
    assert "nope.txt" in err.value.decode() and b.n == 0 and not b.bt


# ------------------------------------------------------------------------------------------------
# b<q> terms
# ------------------------------------------------------------------------------------------------
def _rules(tmp_path, text, n_pat, n_rel, n_chains, n_hdr, n_bt, how="bt"):
    path = tmp_path / "rules.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Rules()
    err = C.create_string_buffer(_lib.KMP_RULES_ERRBUF)
    p = str(path).encode()
    if how == "bt":
        rc = L.kmp_rules_parse_bt(p, n_pat, n_rel, n_chains, n_hdr, n_bt, C.byref(r), err)
    elif how == "hdr":
        rc = L.kmp_rules_parse_hdr(p, n_pat, n_rel, n_chains, n_hdr, C.byref(r), err)
    elif how == "terms":
        rc = L.kmp_rules_parse_terms(p, n_pat, n_rel, n_chains, C.byref(r), err)
    elif how == "rel":
        rc = L.kmp_rules_parse_rel(p, n_pat, n_rel, C.byref(r), err)
    else:
        rc = L.kmp_rules_parse(p, n_pat, C.byref(r), err)
    if rc:
        assert not r.off and not r.terms and r.n == 0
        return rc, None, err.value.decode()
    try:
        return 0, [[r.terms[j] for j in range(r.off[i], r.off[i + 1])] for i in range(r.n)], err.value.decode()
    finally:
        L.kmp_rules_free(C.byref(r))


def test_rules_with_byte_test_terms(tmp_path):
    # 8 patterns, 2 relations, 1 chain, 4 predicates, 3 byte tests: rows 0..7, 8..9, 10, 11..14, 15..17
    text = b"# all five kinds\n0 b0\n\n!b2 2 r1 c0 h3\r\nb1 !b1 b001\n  !7 \t!b2\n"
    rc, rules, msg = _rules(tmp_path, text, 8, 2, 1, 4, 3)
    assert rc == 0 and msg == ""
    assert rules == [[0, 15], [NOT | 17, 2, 9, 10, 14], [16, NOT | 16, 16], [NOT | 7, NOT | 17]]
    # with nothing else set the tests' rows follow the patterns'
    assert _rules(tmp_path, b"b0 !b1 1\n", 3, 0, 0, 0, 2)[1] == [[3, NOT | 4, 1]]


@pytest.mark.parametrize("text, line, what", [
    (b"0 b3\n", 1, "byte test index 3, but there are 3 byte tests"),
    (b"0\n!b99999999999\n", 2, "byte test index 99999999999"),
    (b"b\n", 1, "'b' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index>"),
    (b"!b\n", 1, "'!b' is not a pattern index"),
    (b"b1x\n", 1, "'b1x' is not a pattern index"),
    (b"bb1\n", 1, "'bb1' is not a pattern index"),
])
def test_refused_byte_test_terms(tmp_path, text, line, what):
    rc, rules, msg = _rules(tmp_path, text, 8, 2, 1, 4, 3)
    assert rc == EINVAL and rules is None
    assert msg.startswith(f"line {line}: ") and what in msg, msg


def test_the_old_entries_know_no_byte_test_terms(tmp_path):
    """kmp_rules_parse, _rel, _terms and _hdr are kmp_rules_parse_bt with no byte tests: "b3" is no term at all, and their messages are
    byte for byte what they were"""
    for how, n_rel, n_chains, n_hdr, tail in (("plain", 0, 0, 0, ""), ("rel", 2, 0, 0, " or r<relation index>"),
                                              ("terms", 2, 1, 0, " or r<relation index> or c<chain index>"),
                                              ("hdr", 2, 1, 4, " or r<relation index> or c<chain index> or h<header index>")):
        rc, rules, msg = _rules(tmp_path, b"0 1\nb3\n", 8, n_rel, n_chains, n_hdr, 0, how)
        assert rc == EINVAL and msg == "line 2: 'b3' is not a pattern index" + tail, msg
    rc, rules, msg = _rules(tmp_path, b"0 b3\n", 8, 2, 1, 4, 0)
    assert rc == EINVAL and msg == "line 1: 'b3' is not a pattern index or r<relation index> or c<chain index> or h<header index>"
    assert _rules(tmp_path, b"!\n", 8, 0, 0, 0, 2)[2] == "line 1: '!' without a pattern index"
    assert _rules(tmp_path, b"0 r1 c0 h2\n", 8, 2, 1, 4, 0, "hdr")[1] == [[0, 9, 10, 13]]
    assert _rules(tmp_path, b"9\n", 8, 0, 0, 0, 2)[2] == "line 1: pattern index 9, but there are 8 patterns"


def test_too_many_rows_for_a_term(tmp_path):
    rc, rules, msg = _rules(tmp_path, b"0\n", (1 << 31) - 6, 1, 1, 2, 2)
    assert rc == EINVAL and "line" not in msg
    assert msg == "2147483642 patterns + 1 relations + 1 chains + 2 header predicates + 2 byte tests do not fit the 2^31 rows a term can name"
    assert _rules(tmp_path, b"0 b1\n", (1 << 31) - 7, 1, 1, 2, 2)[1] == [[0, (1 << 31) - 2]]
    # without byte tests the message is the headers' own
    rc, rules, msg = _rules(tmp_path, b"0\n", (1 << 31) - 4, 1, 1, 2, 0)
    assert rc == EINVAL and msg == "2147483644 patterns + 1 relations + 1 chains + 2 header predicates do not fit the 2^31 rows a term can name"


# ------------------------------------------------------------------------------------------------
# the packers and the parsers under sanitizers
# ------------------------------------------------------------------------------------------------
def test_byte_test_packers_and_parsers_under_sanitizers(tmp_path):
    """csrc/kmp_rowtables.cpp and csrc/host/kmphost.c under ASan + UBSan in a stand-alone program, tests/bytetests_sanitizer_driver.cpp: the
    tests' device records, every KMPGPU_EINVAL case, the 2^31 bounds, the n_bt entries of the other packers, and the two parsers on files."""
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no gcc / g++")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    host_o, exe = str(tmp_path / "kmphost.o"), str(tmp_path / "bytetests_driver")
    subprocess.run(["gcc", "-std=gnu11", "-fopenmp", *san, *inc, "-c", os.path.join(CSRC, "host", "kmphost.c"), "-o", host_o],
                   check=True, capture_output=True, timeout=300)
    subprocess.run(["g++", "-std=c++17", "-fopenmp", *san, *inc, os.path.join(ROOT, "tests", "bytetests_sanitizer_driver.cpp"),
                    os.path.join(CSRC, "kmp_rowtables.cpp"), host_o, "-o", exe], check=True, capture_output=True, timeout=300)
    good, bad, rules = tmp_path / "good.txt", tmp_path / "bad.txt", tmp_path / "rules.txt"
    good.write_bytes(b"2 & 0x8000 2\n" + b"".join(b"%d >= %d %d after %d little mask 0x%x\n" % (1 + i % 4, i, i - 50, i % 3, i) for i in range(130)))
    bad.write_bytes(b"2 = 1 4\n" * 70 + b"2 = 1 4 after 3\n")
    rules.write_bytes(b"b130 !b0 1\n0 b7\n")
    r = subprocess.run([exe, str(good), str(bad), str(rules)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "bytetests driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
