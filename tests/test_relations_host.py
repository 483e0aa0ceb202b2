"""The relation parsers of the host library (kmp_relations_parse, kmp_rules_parse_rel, include/kmphost.h): no GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from multithreading_string_matching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NOT = _lib.RULE_NOT
EIO, EINVAL = -1, -4                                   # KMPHOST_EIO, KMPHOST_EINVAL


def _relations(tmp_path, text, n_patterns):
    """(rc, [(a, b, dmin, dmax)] or None, message)"""
    path = tmp_path / "relations.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Relations()
    err = C.create_string_buffer(_lib.KMP_RELATIONS_ERRBUF)
    rc = L.kmp_relations_parse(str(path).encode(), n_patterns, C.byref(r), err)
    if rc:
        assert not r.rel and r.n == 0                  # nothing is handed out on failure
        return rc, None, err.value.decode()
    try:
        rels = [(r.rel[q].a, r.rel[q].b, r.rel[q].dmin, r.rel[q].dmax) for q in range(r.n)]
    finally:
        L.kmp_relations_free(C.byref(r))
    return 0, rels, err.value.decode()


def _rules(tmp_path, text, n_patterns, n_relations, plain=False):
    """(rc, the rules as lists of terms or None, message)"""
    path = tmp_path / "rules.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Rules()
    err = C.create_string_buffer(_lib.KMP_RULES_ERRBUF)
    if plain:
        rc = L.kmp_rules_parse(str(path).encode(), n_patterns, C.byref(r), err)
    else:
        rc = L.kmp_rules_parse_rel(str(path).encode(), n_patterns, n_relations, C.byref(r), err)
    if rc:
        assert not r.off and not r.terms and r.n == 0
        return rc, None, err.value.decode()
    try:
        rules = [[r.terms[j] for j in range(r.off[i], r.off[i + 1])] for i in range(r.n)]
    finally:
        L.kmp_rules_free(C.byref(r))
    return 0, rules, err.value.decode()


GOOD_RELATIONS = (b"# a b dmin dmax\n"
                  b"\n"
                  b"0 1 0 20\n"
                  b"   \t \n"
                  b"\t3\t3  -7 -7 \r\n"
                  b"  # indented comment 1 2 3 4\n"
                  b"5 0 * 12\n"
                  b"0002 007 -40 *\n"
                  b"6 6 * *\n"
                  b"1 0 -2147483648 2147483647\n"
                  b"1 0 -2147483647 2147483646\n"
                  b"4 2 -0 0")                                     # last line without a newline
GOOD_PARSED = [(0, 1, 0, 20), (3, 3, -7, -7), (5, 0, I32_MIN, 12), (2, 7, -40, I32_MAX), (6, 6, I32_MIN, I32_MAX), (1, 0, I32_MIN, I32_MAX),
               (1, 0, I32_MIN + 1, I32_MAX - 1), (4, 2, 0, 0)]
GOOD_RULES = (b"# signatures over patterns and relations\n"
              b"0 1 r0\n"
              b"\n"
              b"!r7 3\r\n"
              b"r1 !r1 r001\n"
              b"  !2 \t!r3  \n"
              b"7 r7")


def test_good_relations_file(tmp_path):
    rc, rels, msg = _relations(tmp_path, GOOD_RELATIONS, 8)
    assert rc == 0 and msg == ""
    assert rels == GOOD_PARSED


def test_empty_and_comment_only_files(tmp_path):
    for text in (b"", b"\n\n", b"# nothing\n   # here\n"):
        rc, rels, _ = _relations(tmp_path, text, 3)
        assert rc == 0 and rels == []


def test_many_relations(tmp_path):
    n = 5000
    text = b"".join(b"%d %d %d %d\n" % (i % 9, (i * 7) % 9, -(i % 50), i % 31) for i in range(n))
    rc, rels, _ = _relations(tmp_path, text, 9)
    assert rc == 0 and rels == [(i % 9, (i * 7) % 9, -(i % 50), i % 31) for i in range(n)]


@pytest.mark.parametrize("text, line, what", [
    (b"0 1 0 5\n5 0 0 0\n", 2, "5"),                              # a >= n_patterns
    (b"0 1 0 5\n\n0 5 0 0\n", 3, "5"),                            # b >= n_patterns
    (b"# c\n\n99999999999 0 0 0\n", 3, "99999999999"),            # ... far beyond, and beyond 32 bits
    (b"0 1 0 5\n1 2 9 8\n", 2, "9"),                              # dmin > dmax
    (b"1 1 1 0", 1, "1"),                                         # ... at the end of a file without a newline
    (b"1 1 -3 -4\n", 1, "-3"),
    (b"0 0 0 0\nabc 0 0 0\n", 2, "abc"),                          # a field that is not a number: an index,
    (b"0 x1 0 5\n", 1, "x1"),
    (b"0 1 5x 6\n", 1, "5x"),                                     # a bound (digits, then something else)
    (b"0 1 5 --6\n", 1, "--6"),
    (b"0 1 - 6\n", 1, "'-'"),
    (b"-1 1 0 6\n", 1, "-1"),                                     # an index has no sign
    (b"* 1 0 5\n", 1, "*"),                                       # '*' stands for a bound only
    (b"0 * 0 5\n", 1, "*"),
    (b"0 1 ** 5\n", 1, "**"),
    (b"0 1 0 2147483648\n", 1, "2147483648"),                     # does not fit 32 bits
    (b"0 1 -2147483649 0\n", 1, "-2147483649"),
    (b"1 2 3\n", 1, "four fields"),                               # a field is missing
    (b"# c\n1\n", 2, "four fields"),
    (b"1 2 3 4 5\n", 1, "four fields"),                           # one too many
])
def test_relation_errors_carry_the_line_number(tmp_path, text, line, what):
    rc, rels, msg = _relations(tmp_path, text, 5)
    assert rc == EINVAL and rels is None
    assert msg.startswith(f"line {line}: "), msg
    assert what in msg, msg


def test_missing_relations_file(tmp_path):
    L = _lib.host_lib()
    r = _lib.Relations()
    err = C.create_string_buffer(_lib.KMP_RELATIONS_ERRBUF)
    assert L.kmp_relations_parse(str(tmp_path / "none.txt").encode(), 3, C.byref(r), err) == EIO
    assert err.value and not r.rel and r.n == 0


def test_rules_with_relation_terms(tmp_path):
    n = 10
    rc, rules, msg = _rules(tmp_path, GOOD_RULES, n, 8)
    assert rc == 0 and msg == ""
    assert rules == [[0, 1, n + 0], [(n + 7) | NOT, 3], [n + 1, (n + 1) | NOT, n + 1], [2 | NOT, (n + 3) | NOT], [7, n + 7]]
    # without relation terms the two parsers agree, whatever n_relations is
    text = b"0 1 !2\n# c\n!0 !1\n9\n"
    want = [[0, 1, 2 | NOT], [0 | NOT, 1 | NOT], [9]]
    assert _rules(tmp_path, text, n, 0)[1] == _rules(tmp_path, text, n, 8)[1] == _rules(tmp_path, text, n, 0, plain=True)[1] == want


@pytest.mark.parametrize("text, line, what", [
    (b"0 r0\nr8\n", 2, "8"),                                      # relation index >= n_relations
    (b"0\n\n!r99999999999\n", 3, "99999999999"),
    (b"r\n", 1, "'r'"),                                           # no index
    (b"0 !r\n", 1, "!r"),
    (b"r1x\n", 1, "r1x"),
    (b"rr1\n", 1, "rr1"),
    (b"R1\n", 1, "R1"),
    (b"r-1\n", 1, "r-1"),
    (b"0 r1\n1 10\n", 2, "10"),                                   # a pattern index >= n_patterns stays an error
    (b"!!r1\n", 1, "!!r1"),
])
def test_rule_errors_with_relations(tmp_path, text, line, what):
    rc, rules, msg = _rules(tmp_path, text, 10, 8)
    assert rc == EINVAL and rules is None
    assert msg.startswith(f"line {line}: "), msg
    assert what in msg, msg


def test_rows_have_to_fit_31_bits(tmp_path):
    """n_patterns + n_relations >= 2^31: a term would reach KMP_RULE_NOT's bit, or wrap"""
    for n_pat, n_rel in ((10, (1 << 31) - 10), (1 << 30, 1 << 30), (0xFFFFFFFF, 0xFFFFFFFF), (1 << 31, 0), (5, 0xFFFFFFFF)):
        rc, rules, msg = _rules(tmp_path, b"0 r0\n", n_pat, n_rel)
        assert rc == EINVAL and rules is None and "2^31" in msg and not msg.startswith("line"), (n_pat, n_rel, msg)
    rc, rules, _ = _rules(tmp_path, b"0 !r0 r5\n", 10, (1 << 31) - 11)          # the largest set that fits
    assert rc == 0 and rules == [[0, 10 | NOT, 15]]
    rc, rules, _ = _rules(tmp_path, b"r%d !r%d\n" % ((1 << 31) - 12, (1 << 31) - 12), 10, (1 << 31) - 11)
    assert rc == 0 and rules == [[(1 << 31) - 2, ((1 << 31) - 2) | NOT]]


def test_plain_rules_parser_still_rejects_relation_terms(tmp_path):
    for plain in (True, False):
        rc, rules, msg = _rules(tmp_path, b"0 1\n2 r0\n", 10, 0, plain=plain)
        assert rc == EINVAL and rules is None
        assert msg.startswith("line 2: ") and "r0" in msg, msg
    rc, _, msg = _rules(tmp_path, b"r3\n", 10, 0, plain=True)
    assert rc == EINVAL and msg.startswith("line 1: ") and "r3" in msg


# ---- the parsers under AddressSanitizer + UBSan: a stand-alone program, tests/relations_sanitizer_driver.c ---
def test_relation_parsers_under_sanitizers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "relations_driver")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-fopenmp", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "relations_sanitizer_driver.c"),
           os.path.join(ROOT, "multithreading_string_matching_amd", "csrc", "host", "kmphost.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0 and "relations driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
        return r.stdout.splitlines()

    lf, rf = tmp_path / "relations.txt", tmp_path / "rules.txt"
    lf.write_bytes(GOOD_RELATIONS)
    rf.write_bytes(GOOD_RULES)
    out = run("10", str(lf), str(rf))
    assert out[0] == f"relations rc=0 n={len(GOOD_PARSED)} msg="
    assert out[1:1 + len(GOOD_PARSED)] == [f"rel {a} {b} {lo} {hi}" for a, b, lo, hi in GOOD_PARSED]
    assert out[1 + len(GOOD_PARSED)] == "rules rc=0 n=5 msg="
    assert out[2 + len(GOOD_PARSED)] == "rule 0 1 10"
    assert out[-2].startswith(f"plain rc={EINVAL} msg=line 2: ")
    # every error path, and long lines
    bad = [b"0 1 9 3\n", b"0 1 0\n", b"0 1 0 5 6\n", b"0 99 0 5\n", b"x 1 0 5\n", b"0 1 * 99999999999999999999\n", b"0 1 0 5\n" * 300 + b"0 1 5 4",
           b"0 1 0 " + b"7" * 5000 + b"\n", b"# " + b"c" * 70000 + b"\n0 1 -5 5\n" + b" " * 70000 + b"1 0 * *"]
    for i, text in enumerate(bad):
        lf.write_bytes(text)
        out = run("10", str(lf), str(rf))
        assert out[0].startswith("relations rc=0 n=2 msg=" if i == len(bad) - 1 else f"relations rc={EINVAL} n=0 msg=line "), out[0]
    lf.write_bytes(GOOD_RELATIONS)
    for text in (b"r8\n", b"0 1\n!r\n", b"r0 " * 3000 + b"\n" + b"!r7\n" * 3000, b"r" + b"1" * 300 + b"\n", b"0 rx\n", b""):
        rf.write_bytes(text)
        out = run("10", str(lf), str(rf))
        assert any(line.startswith("rules rc=") for line in out)
    assert run("10", str(tmp_path / "none.txt"), str(tmp_path / "none2.txt"))[0].startswith(f"relations rc={EIO} n=0")
