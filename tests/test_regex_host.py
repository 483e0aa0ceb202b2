"""The host side of the regex rows: the compiler and the interpreter of csrc/kmp_regex.cpp (kmp_regex_compile, kmp_regex_search), held to
tests/regex_model.py -- Python's re -- on random short strings, kmp_pack_regexes and the n_rx entries of the other packers, all under
ASan + UBSan in a stand-alone program (tests/regex_sanitizer_driver.cpp).  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import regex_model as RM
from multithreading_string_matching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")

# every element form, every quantifier form, both anchors; each is run under all four flag combinations
ACCEPTED = [
    b"a", b"ab", b"a.b", b"[^a]b", b"[^a]", b"^\\s*$", b"ab{0,2}$", b"a.{0,3}b", b"a{3,}", b"\\d\\D", b"\\w\\W", b"\\S\\s", b"[a7]{2}",
    b"[^\\n]{5}", b"a?b+7*=", b"^a", b"7$", b"^[aAb7 =]+$", b"\\x80+", b"\x80a", b"[\\x00-\\x20]{2}", b"a\\x00", b"\\0b", b"=\\s?a",
    b"[a-b]{2,3}7", b"\\n.", b"[\\d\\s]+=$", b"^b*$", b"a+b?", b"\\=[ ]*\\w", b"[^\\Wa]", b"A", b"[-a]7", b"[a\\-]7", b"[7-]a",
    b"[\\t\\r\\f\\v ]a", b"a{2}", b"a{1,2}b", b"a{2,}b", b"^.{3}$", b".{0,2}\\x80$", b"[\\]\\\\a]b", b"\\D{4}7", b"^\\W", b"\\S{3,5}$",
]
# ... and the ones that match the empty string: every text, named as such
ALL_TRUE = [b"b*", b"a?", b"7{0,3}", b"\\s*$", b"^\\d*"]
ALPHABET = b"\n\0aAb7 \x80="
LENGTHS = (0, 1, 2, 3, 5, 8, 13, 17)


def test_constants():
    assert (_lib.RX_NOCASE, _lib.RX_DOTALL, _lib.RX_GATED) == (RM.NOCASE, RM.DOTALL, RM.GATED) == (1, 2, 4)
    text = open(os.path.join(ROOT, "include", "kmpgpu.h")).read()
    for name, value in (("KMPGPU_RX_NOCASE", "1u"), ("KMPGPU_RX_DOTALL", "2u"), ("KMPGPU_RX_GATED", "4u"),
                        ("KMPGPU_RX_MAX_POSITIONS", str(_lib.RX_MAX_POSITIONS))):
        assert any(line.split()[:3] == ["#define", name, value] for line in text.splitlines()), name
    assert f"#define KMP_RX_TILE {_lib.RX_TILE}u" in open(os.path.join(CSRC, "kmp_regex.h")).read()


def _texts():
    rng = np.random.default_rng(20261019)
    alphabet = np.frombuffer(ALPHABET, dtype=np.uint8)
    return [bytes(rng.choice(alphabet, n)) for n in LENGTHS for _ in range(300)]


def test_compiler_interpreter_and_packers_under_sanitizers(tmp_path):
    """the model's verdicts first -- none of the accepted expressions is trivially all-true or all-false on these texts, but the ones
    named as such -- then the driver, which must give the same verdict on every (expression, flags, rule, text)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    texts = _texts()
    assert len(texts) >= 2000
    lines = ["S " + (t.hex() or "-") for t in texts]
    n_expr = 0
    for expr in ACCEPTED + ALL_TRUE:
        for flags in range(4):
            nocase, dotall = bool(flags & RM.NOCASE), bool(flags & RM.DOTALL)
            lines.append(f"X {flags} {expr.hex()}")
            both = []
            for whole in (False, True):
                v = [RM.search(expr, t, nocase, dotall, whole) for t in texts]
                both += v
                lines.append(f"V {int(whole)} " + "".join("01"[x] for x in v))
            if expr in ALL_TRUE:
                assert all(both), expr
            else:
                assert any(both) and not all(both), (expr, flags)
            n_expr += 1
    assert n_expr >= 30 * 4
    verdicts = tmp_path / "verdicts.txt"
    verdicts.write_text("\n".join(lines) + "\n")

    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    exe = str(tmp_path / "regex_driver")
    subprocess.run(["g++", "-std=c++17", *san, *inc, os.path.join(ROOT, "tests", "regex_sanitizer_driver.cpp"),
                    os.path.join(CSRC, "kmp_regex.cpp"), os.path.join(CSRC, "kmp_rowtables.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, str(verdicts)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "regex driver ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert f"{n_expr} expressions, {len(texts)} texts, {n_expr * 2 * len(texts)} verdicts" in r.stdout
