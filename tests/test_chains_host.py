"""The chain parsers of the host library (kmp_chains_parse, kmp_rules_parse_terms, include/kmphost.h): no GPU needed."""
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


def _chains(tmp_path, text, n_patterns):
    """(rc, [[(pattern, dmin, dmax), ...]] or None, message)"""
    path = tmp_path / "chains.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Chains()
    err = C.create_string_buffer(_lib.KMP_CHAINS_ERRBUF)
    rc = L.kmp_chains_parse(str(path).encode(), n_patterns, C.byref(r), err)
    if rc:
        assert not r.off and not r.links and r.n == 0   # nothing is handed out on failure
        return rc, None, err.value.decode()
    try:
        chains = [[(r.links[j].pattern, r.links[j].dmin, r.links[j].dmax) for j in range(r.off[c], r.off[c + 1])] for c in range(r.n)]
    finally:
        L.kmp_chains_free(C.byref(r))
    return 0, chains, err.value.decode()


def _rules(tmp_path, text, n_patterns, n_relations, n_chains, how="terms"):
    """(rc, the rules as lists of terms or None, message)"""
    path = tmp_path / "rules.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Rules()
    err = C.create_string_buffer(_lib.KMP_RULES_ERRBUF)
    if how == "terms":
        rc = L.kmp_rules_parse_terms(str(path).encode(), n_patterns, n_relations, n_chains, C.byref(r), err)
    elif how == "rel":
        rc = L.kmp_rules_parse_rel(str(path).encode(), n_patterns, n_relations, C.byref(r), err)
    else:
        rc = L.kmp_rules_parse(str(path).encode(), n_patterns, C.byref(r), err)
    if rc:
        assert not r.off and not r.terms and r.n == 0
        return rc, None, err.value.decode()
    try:
        rules = [[r.terms[j] for j in range(r.off[i], r.off[i + 1])] for i in range(r.n)]
    finally:
        L.kmp_rules_free(C.byref(r))
    return 0, rules, err.value.decode()


OPEN = (I32_MIN, I32_MAX)
GOOD_CHAINS = (b"# p0 dmin dmax p1 [dmin dmax p2 ...]\n"
               b"\n"
               b"0 0 20 1\n"
               b"   \t \n"
               b"\t3\t-7 -7  3 \r\n"
               b"  # indented comment 1 2 3 4\n"
               b"5 * 12 0 0 * 2\n"
               b"0002 -40 * 007 * * 1 -2147483648 2147483647 1\n"
               b"1 0 0 1 0 0 1 0 0 1 0 0 1 0 0 1 0 0 1 0 0 1\n"
               b"4 -0 0 2")                                         # last line without a newline
GOOD_PARSED = [[(0, *OPEN), (1, 0, 20)], [(3, *OPEN), (3, -7, -7)], [(5, *OPEN), (0, I32_MIN, 12), (2, 0, I32_MAX)],
               [(2, *OPEN), (7, -40, I32_MAX), (1, *OPEN), (1, *OPEN)], [(1, *OPEN)] + [(1, 0, 0)] * 7, [(4, *OPEN), (2, 0, 0)]]
GOOD_RULES = (b"# signatures over patterns, relations and chains\n"
              b"0 1 c0\n"
              b"\n"
              b"!c5 3 r2\r\n"
              b"c1 !c1 c001\n"
              b"  !2 \t!c3  !r0\n"
              b"7 c5")


def test_good_chains_file(tmp_path):
    rc, chains, msg = _chains(tmp_path, GOOD_CHAINS, 8)
    assert rc == 0 and msg == ""
    assert chains == GOOD_PARSED


def test_empty_and_comment_only_files(tmp_path):
    for text in (b"", b"\n\n", b"# nothing\n   # here\n"):
        rc, chains, _ = _chains(tmp_path, text, 3)
        assert rc == 0 and chains == []


def test_many_chains(tmp_path):
    n = 3000
    text = b"".join(b"%d %d %d %d %d * %d\n" % (i % 9, -(i % 50), i % 31, (i * 7) % 9, i % 5, (i * 5) % 9) for i in range(n))
    rc, chains, _ = _chains(tmp_path, text, 9)
    assert rc == 0 and chains == [[(i % 9, *OPEN), ((i * 7) % 9, -(i % 50), i % 31), ((i * 5) % 9, i % 5, I32_MAX)] for i in range(n)]


@pytest.mark.parametrize("text, line, what", [
    (b"0 0 5 1\n5 0 0 0\n", 2, "5"),                              # p0 >= n_patterns
    (b"0 0 5 1\n\n0 0 0 5\n", 3, "5"),                            # p1 >= n_patterns
    (b"0 0 5 1 0 0 7\n", 1, "7"),                                 # p2
    (b"# c\n\n99999999999 0 0 0\n", 3, "99999999999"),            # ... far beyond, and beyond 32 bits
    (b"0 0 5 1\n1 9 8 2\n", 2, "9"),                              # dmin > dmax
    (b"1 1 0 1", 1, "1"),                                         # ... at the end of a file without a newline
    (b"1 0 0 1 -3 -4 1\n", 1, "-3"),                              # ... on a later link
    (b"0 0 0 0\nabc 0 0 0\n", 2, "abc"),                          # a field that is not a number: an index,
    (b"0 0 5 x1\n", 1, "x1"),
    (b"0 5x 6 1\n", 1, "5x"),                                     # a bound (digits, then something else)
    (b"0 5 --6 1\n", 1, "--6"),
    (b"0 - 6 1\n", 1, "'-'"),
    (b"-1 0 6 1\n", 1, "-1"),                                     # an index has no sign
    (b"* 0 5 1\n", 1, "*"),                                       # '*' stands for a bound only
    (b"0 0 5 *\n", 1, "*"),
    (b"0 ** 5 1\n", 1, "**"),
    (b"0 0 2147483648 1\n", 1, "2147483648"),                     # does not fit 32 bits
    (b"0 -2147483649 0 1\n", 1, "-2147483649"),
    (b"1\n", 1, "at least 2 contents"),                           # one content
    (b"# c\n1 2\n", 2, "<p0> <dmin> <dmax> <p1>"),                # the field count is not 3n - 2
    (b"1 2 3\n", 1, "<p0> <dmin> <dmax> <p1>"),
    (b"1 2 3 4 0\n", 1, "<p0> <dmin> <dmax> <p1>"),
    (b"1 2 3 4 0 0\n", 1, "<p0> <dmin> <dmax> <p1>"),
    (b"0 0 5 1\n" + b"1" + b" 0 0 1" * 8 + b"\n", 2, "more than 8 contents"),   # nine contents
])
def test_chain_errors_carry_the_line_number(tmp_path, text, line, what):
    rc, chains, msg = _chains(tmp_path, text, 5)
    assert rc == EINVAL and chains is None
    assert msg.startswith(f"line {line}: "), msg
    assert what in msg, msg


def test_missing_chains_file(tmp_path):
    L = _lib.host_lib()
    r = _lib.Chains()
    err = C.create_string_buffer(_lib.KMP_CHAINS_ERRBUF)
    assert L.kmp_chains_parse(str(tmp_path / "none.txt").encode(), 3, C.byref(r), err) == EIO
    assert err.value and not r.off and not r.links and r.n == 0


def test_rules_with_chain_terms(tmp_path):
    n, nr = 10, 4
    rc, rules, msg = _rules(tmp_path, GOOD_RULES, n, nr, 6)
    assert rc == 0 and msg == ""
    b = n + nr
    assert rules == [[0, 1, b + 0], [(b + 5) | NOT, 3, n + 2], [b + 1, (b + 1) | NOT, b + 1], [2 | NOT, (b + 3) | NOT, (n + 0) | NOT], [7, b + 5]]
    # chains without relations: c<q> sits directly behind the patterns, and r<q> is no term
    assert _rules(tmp_path, b"c2 !c0\n", n, 0, 3)[1] == [[n + 2, n | NOT]]
    rc, _, msg = _rules(tmp_path, b"c2 r0\n", n, 0, 3)
    assert rc == EINVAL and msg.startswith("line 1: ") and "r0" in msg
    # without chain terms the parsers agree, whatever n_chains is
    text = b"0 1 !2\n# c\n!0 !r1\n9\n"
    want = [[0, 1, 2 | NOT], [0 | NOT, (n + 1) | NOT], [9]]
    assert _rules(tmp_path, text, n, nr, 0)[1] == _rules(tmp_path, text, n, nr, 6)[1] == _rules(tmp_path, text, n, nr, 0, how="rel")[1] == want


@pytest.mark.parametrize("text, line, what", [
    (b"0 c0\nc6\n", 2, "6"),                                      # chain index >= n_chains
    (b"0\n\n!c99999999999\n", 3, "99999999999"),
    (b"c\n", 1, "'c'"),                                           # no index
    (b"0 !c\n", 1, "!c"),
    (b"c1x\n", 1, "c1x"),
    (b"cc1\n", 1, "cc1"),
    (b"C1\n", 1, "C1"),
    (b"c-1\n", 1, "c-1"),
    (b"rc1\n", 1, "rc1"),
    (b"0 c1\n1 10\n", 2, "10"),                                   # a pattern index >= n_patterns stays an error
    (b"0 c1\n1 r4\n", 2, "4"),                                    # ... and so does a relation index >= n_relations
    (b"!!c1\n", 1, "!!c1"),
])
def test_rule_errors_with_chains(tmp_path, text, line, what):
    rc, rules, msg = _rules(tmp_path, text, 10, 4, 6)
    assert rc == EINVAL and rules is None
    assert msg.startswith(f"line {line}: "), msg
    assert what in msg, msg


def test_rows_have_to_fit_31_bits(tmp_path):
    """n_patterns + n_relations + n_chains >= 2^31: a term would reach KMP_RULE_NOT's bit, or wrap"""
    for n_pat, n_rel, n_ch in ((10, 5, (1 << 31) - 15), (1 << 30, 1 << 29, 1 << 29), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (5, 0, 0xFFFFFFFF),
                               (10, (1 << 31) - 11, 1), (1, 0xFFFFFFFF, 0xFFFFFFFF)):
        rc, rules, msg = _rules(tmp_path, b"0 c0\n", n_pat, n_rel, n_ch)
        assert rc == EINVAL and rules is None and "2^31" in msg and not msg.startswith("line"), (n_pat, n_rel, n_ch, msg)
    rc, rules, _ = _rules(tmp_path, b"0 !c0 c5 r1\n", 10, 2, (1 << 31) - 13)          # the largest set that fits
    assert rc == 0 and rules == [[0, 12 | NOT, 17, 11]]
    rc, rules, _ = _rules(tmp_path, b"c%d !c%d\n" % ((1 << 31) - 14, (1 << 31) - 14), 10, 2, (1 << 31) - 13)
    assert rc == 0 and rules == [[(1 << 31) - 2, ((1 << 31) - 2) | NOT]]


def test_relation_parser_still_rejects_chain_terms(tmp_path):
    for how in ("rel", "terms"):
        rc, rules, msg = _rules(tmp_path, b"0 1 r0\n2 c0\n", 10, 4, 0, how=how)
        assert rc == EINVAL and rules is None
        assert msg.startswith("line 2: ") and "c0" in msg, msg
    rc, _, msg = _rules(tmp_path, b"c3\n", 10, 0, 0, how="plain")
    assert rc == EINVAL and msg.startswith("line 1: ") and "c3" in msg


# ---- the parsers under AddressSanitizer + UBSan: a stand-alone program, tests/chains_sanitizer_driver.c ---
def test_chain_parsers_under_sanitizers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "chains_driver")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-fopenmp", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "chains_sanitizer_driver.c"),
           os.path.join(ROOT, "multithreading_string_matching_amd", "csrc", "host", "kmphost.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0 and "chains driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
        return r.stdout.splitlines()

    cf, rf = tmp_path / "chains.txt", tmp_path / "rules.txt"
    cf.write_bytes(GOOD_CHAINS)
    rf.write_bytes(GOOD_RULES)
    out = run("10", "4", str(cf), str(rf))
    assert out[0] == f"chains rc=0 n={len(GOOD_PARSED)} msg="
    assert out[1:1 + len(GOOD_PARSED)] == ["chain " + " ".join(f"{lo} {hi} {p}" for p, lo, hi in ch) for ch in GOOD_PARSED]
    assert out[1 + len(GOOD_PARSED)] == "rules rc=0 n=5 msg="
    assert out[2 + len(GOOD_PARSED)] == "rule 0 1 14"
    assert out[-2].startswith(f"rel rc={EINVAL} msg=line 2: ")            # (c0 is no term without chains)
    # every error path, and long lines
    bad = [b"0 9 3 1\n", b"0 1 0\n", b"0 0 5 1 6\n", b"0 0 5 99\n", b"x 0 5 1\n", b"0 * 99999999999999999999 1\n", b"0 0 5 1\n" * 300 + b"0 5 4 1",
           b"0 0 " + b"7" * 5000 + b" 1\n", b"1" + b" 0 0 1" * 8 + b"\n", b"1" + b" 0 0 1" * 4000 + b"\n", b"1\n",
           b"# " + b"c" * 70000 + b"\n0 -5 5 1\n" + b" " * 70000 + b"1 * * 0 * * 2"]
    for i, text in enumerate(bad):
        cf.write_bytes(text)
        out = run("10", "4", str(cf), str(rf))
        assert out[0].startswith("chains rc=0 n=2 msg=" if i == len(bad) - 1 else f"chains rc={EINVAL} n=0 msg=line "), out[0]
    cf.write_bytes(GOOD_CHAINS)
    for text in (b"c6\n", b"0 1\n!c\n", b"c0 " * 3000 + b"\n" + b"!c5\n" * 3000, b"c" + b"1" * 300 + b"\n", b"0 cx\n", b""):
        rf.write_bytes(text)
        out = run("10", "4", str(cf), str(rf))
        assert any(line.startswith("rules rc=") for line in out)
    assert run("10", "4", str(tmp_path / "none.txt"), str(tmp_path / "none2.txt"))[0].startswith(f"chains rc={EIO} n=0")
