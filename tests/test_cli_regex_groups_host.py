"""The flag letter e of an expressions file (kmp_regexes_parse, include/kmphost.h): KMP_RX_GROUPS.  No GPU needed."""
import pytest

from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.host import KmpHostError, parse_regexes


def test_flag_letter_e(tmp_path):
    f = tmp_path / "regex.txt"
    f.write_bytes(b"/(GET|POST) \\//e\n/(a|b)/ie with 0\n/a.b/s\n/x/se with 2\n")
    got = parse_regexes(str(f), 3)
    assert got == [(b"(GET|POST) \\/", {"groups": True}), (b"(a|b)", {"nocase": True, "groups": True, "gate": 0}),
                   (b"a.b", {"dotall": True}), (b"x", {"dotall": True, "groups": True, "gate": 2})]
    assert _lib.RX_GROUPS == 16


@pytest.mark.parametrize("text,what", [("/a/ee\n", "line 1: flag 'e' twice"), ("/a/g\n", "line 1: 'g' is not a flag (i: nocase, s: dotall)"),
                                       ("/a/ex\n", "line 1: 'x' is not a flag (i: nocase, s: dotall)")])
def test_refused_letters(tmp_path, text, what):
    f = tmp_path / "regex.txt"
    f.write_text(text)
    with pytest.raises(KmpHostError) as e:
        parse_regexes(str(f), 1)
    assert what in str(e.value)
