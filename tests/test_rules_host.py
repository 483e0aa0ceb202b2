"""The rules file parser of the host library (kmp_rules_parse, include/kmphost.h): no GPU needed."""
import ctypes as C

import pytest

from multithreading_string_matching_amd import _lib


def _parse(tmp_path, text, n_patterns):
    """(rc, the rules as lists of terms or None, message)"""
    path = tmp_path / "rules.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Rules()
    err = C.create_string_buffer(_lib.KMP_RULES_ERRBUF)
    rc = L.kmp_rules_parse(str(path).encode(), n_patterns, C.byref(r), err)
    if rc:
        assert not r.off and not r.terms and r.n == 0           # nothing is handed out on failure
        return rc, None, err.value.decode()
    try:
        assert r.off[0] == 0
        rules = [[r.terms[j] for j in range(r.off[i], r.off[i + 1])] for i in range(r.n)]
    finally:
        L.kmp_rules_free(C.byref(r))
    return 0, rules, err.value.decode()


NOT = _lib.RULE_NOT


def test_good_file(tmp_path):
    text = (b"# signatures\n"
            b"\n"
            b"0 1 !2\n"
            b"   \t \n"
            b"\t3\t!4  5 \r\n"
            b"  # indented comment 99 !\n"
            b"!0 !1\n"
            b"7 7 !7 7\n"
            b"00012\n"
            b"9 !9")                                               # last line without a newline
    rc, rules, msg = _parse(tmp_path, text, 13)
    assert rc == 0 and msg == ""
    assert rules == [[0, 1, 2 | NOT], [3, 4 | NOT, 5], [0 | NOT, 1 | NOT], [7, 7, 7 | NOT, 7], [12], [9, 9 | NOT]]


def test_empty_and_comment_only_files(tmp_path):
    for text in (b"", b"\n\n", b"# nothing\n   # here\n"):
        rc, rules, _ = _parse(tmp_path, text, 5)
        assert rc == 0 and rules == []


def test_long_rule_and_many_rules(tmp_path):
    text = b" ".join(b"%d" % (i % 7) for i in range(5000)) + b"\n" + b"".join(b"!%d\n" % (i % 7) for i in range(3000))
    rc, rules, _ = _parse(tmp_path, text, 7)
    assert rc == 0 and len(rules) == 3001
    assert rules[0] == [i % 7 for i in range(5000)]
    assert rules[1:] == [[(i % 7) | NOT] for i in range(3000)]


@pytest.mark.parametrize("text, line, what", [
    (b"0 1\nabc\n", 2, "abc"),                                    # not a number
    (b"0 1\n\n# c\n1 2x 0\n", 4, "2x"),                           # digits, then something else
    (b"-1\n", 1, "-1"),
    (b"0\n1 !!2\n", 2, "!!2"),
    (b"0 !x\n", 1, "!x"),
    (b"0\n1\n2 5\n", 3, "5"),                                     # index >= n_patterns
    (b"0\n!5\n", 2, "5"),
    (b"99999999999999999999999\n", 1, "pattern"),                 # far beyond any index
    (b"# c\n0 ! 1\n", 2, "'!'"),                                  # a bare '!'
    (b"0\n1\n\n2 !", 4, "'!'"),                                   # ... at the end of a file without a newline
])
def test_errors_carry_the_line_number(tmp_path, text, line, what):
    rc, rules, msg = _parse(tmp_path, text, 5)
    assert rc == -4 and rules is None                              # KMPHOST_EINVAL
    assert msg.startswith(f"line {line}: "), msg
    assert what in msg, msg


def test_missing_file(tmp_path):
    L = _lib.host_lib()
    r = _lib.Rules()
    err = C.create_string_buffer(_lib.KMP_RULES_ERRBUF)
    assert L.kmp_rules_parse(str(tmp_path / "none.txt").encode(), 3, C.byref(r), err) == -1       # KMPHOST_EIO
    assert err.value
