"""tests/regex_model.py held to verdicts written out by hand from the contract in include/kmpgpu.h (kmpgpu_set_regexes): no GPU, nothing
of the library."""
import numpy as np
import pytest

import regex_model as RM

# (expression, options, text, verdict under the default rule (text ends at the first 0x00), verdict on whole payloads)
HAND = [
    # $ is the text end alone, not "or in front of a final newline"
    (b"a$", {}, b"a\n", False, False),
    (b"a$", {}, b"ba", True, True),
    (b"a\\n$", {}, b"a\n", True, True),
    (b"\\$$", {}, b"x$", True, True),                     # an escaped $ and the anchor behind it
    (b"a\\$", {}, b"a$b", True, True),                    # ... and an escaped $ alone is a literal, no anchor
    # nocase closes the listed set under case BEFORE the negation
    (b"[^a]", {"nocase": True}, b"A", False, False),
    (b"[^a]", {}, b"A", True, True),
    (b"[^a]", {"nocase": True}, b"Ab", True, True),
    (b"abc", {"nocase": True}, b"xAbC", True, True),
    (b"[a-c]x", {"nocase": True}, b"BX", True, True),
    # the dot and 0x0A
    (b".", {}, b"\n", False, False),
    (b".", {"dotall": True}, b"\n", True, True),
    (b"a.b", {}, b"a\nb", False, False),
    (b"a.b", {"dotall": True}, b"a\nb", True, True),
    # an expression that matches the empty string hits every payload, the empty one included
    (b"x*", {}, b"", True, True),
    (b"x*", {}, b"yyy", True, True),
    (b"^x*$", {}, b"", True, True),
    (b"^x*$", {}, b"xxy", False, False),
    (b"x+", {}, b"", False, False),
    # a 0x00 in front of, inside and behind a match
    (b"ab", {}, b"\0ab", False, True),
    (b"ab", {}, b"a\0b", False, False),
    (b"a.b", {}, b"a\0b", False, True),
    (b"a\\x00b", {}, b"a\0b", False, True),
    (b"a\\Db", {}, b"a\0b", False, True),
    (b"a[^x]b", {}, b"a\0b", False, True),
    (b"ab", {}, b"ab\0", True, True),
    (b"ab$", {}, b"ab\0", True, False),                  # the text ends in front of the 0x00, or behind it
    (b"ab$", {}, b"ab\0ab", True, True),
    (b"^ab", {}, b"\0ab", False, False),
    (b"^\\0ab", {}, b"\0ab", False, True),
    # anchors, classes and counts
    (b"^ab", {}, b"cab", False, False),
    (b"\\d{8,}", {}, b"id=1234567", False, False),
    (b"\\d{8,}", {}, b"id=12345678;", True, True),
    (b"= ?\\w", {}, b"k= v", True, True),
    (b"\\s*=\\s*", {}, b"k \t= v", True, True),
    (b"^[0-9a-fA-F]+$", {}, b"deadBEEF", True, True),
    (b"^[0-9a-fA-F]+$", {}, b"deadBEEFx", False, False),
    (b"User-Agent: [^\\n]{4,}", {}, b"User-Agent: abc\nxyz", False, False),
    (b"User-Agent: [^\\n]{4,}", {}, b"User-Agent: abcd\n", True, True),
    (b"a{2,3}b", {}, b"ab", False, False),
    (b"a{2,3}b", {}, b"aaaab", True, True),
    (b"^a{2,3}b", {}, b"aaaab", False, False),
    (b"[\\]\\\\-]", {}, b"x]y", True, True),
    (b"[a\\-c]", {}, b"b", False, False),
    (b"\\x80\xff", {}, b"\x80\xff", True, True),
    (b"\\W\\S", {}, b"ab ", False, False),
    (b"\\W\\S", {}, b"a b", True, True),
]


@pytest.mark.parametrize("expr, opt, text, default, whole", HAND)
def test_hand_written_verdicts(expr, opt, text, default, whole):
    assert RM.search(expr, text, opt.get("nocase", False), opt.get("dotall", False), whole=False) is default
    assert RM.search(expr, text, opt.get("nocase", False), opt.get("dotall", False), whole=True) is whole


def test_rows_and_the_gate():
    payloads = [b"GET /a\n", b"get /b", b"POST\0GET /c", b""]
    exprs = [b"GET /[a-z]", RM.rx(b"GET /[a-z]", nocase=True), RM.rx(b"/[a-z]", gate=1), RM.rx(b"x*", gate=0), b"^$"]
    hits = np.array([[True, False, False, True],          # pattern 0, made up: the gate is the row it is given
                     [False, True, True, False]])
    for whole, want in ((False, [[1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 0, 0], [1, 0, 0, 1], [0, 0, 0, 1]]),
                        (True, [[1, 0, 1, 0], [1, 1, 1, 0], [0, 1, 1, 0], [1, 0, 0, 1], [0, 0, 0, 1]])):
        rows = RM.regex_rows(payloads, exprs, whole=whole, pattern_hits=hits)
        assert rows.dtype == bool and rows.astype(int).tolist() == want, whole


def test_rx_and_parts():
    assert RM.rx(b"a") == b"a"
    assert RM.rx(b"a", nocase=True, gate=0) == (b"a", {"nocase": True, "gate": 0})
    assert RM.parts(b"a") == (b"a", False, False, None)
    assert RM.parts(RM.rx(b"a", dotall=True, gate=3)) == (b"a", False, True, 3)
    assert RM.ends_with_dollar(b"a$") and RM.ends_with_dollar(b"a\\\\$") and not RM.ends_with_dollar(b"a\\$") and not RM.ends_with_dollar(b"a")
