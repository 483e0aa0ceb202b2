"""The host side of the regex rows under KMPGPU_RX_GROUPS: the Glushkov compiler and the interpreter of csrc/kmp_regex.cpp
(kmp_regex_compile_groups, kmp_regex_search_groups), held to tests/regex_model.py -- Python's re -- on random short strings, the refusals,
kmp_pack_regex_groups and the placeholder of kmp_pack_regexes, all under ASan + UBSan in a stand-alone program
(tests/regex_groups_sanitizer_driver.cpp).  No GPU needed."""
import os
import shutil
import subprocess

import pytest

import regex_model as RM
from test_regex_host import ACCEPTED, ALL_TRUE, CSRC, ROOT, _texts
from multithreading_string_matching_amd import _lib

# every new form; each is run under all four flag combinations and both text-end rules.  .{0,60}(a|b)7 has exactly 63 positions,
# ([ab].|7.){2,4}[^=]([aA]|.=) exactly 8 edge rules (the driver checks both counts)
GROUPED = [
    b"a|b7", b"ab|7=|\\x80", b"(a|b)7", b"(a|b|7)=", b"((a|b)7|=)a", b"(a(b|7))+=", b"(ab)?7", b"(ab)*7", b"(ab)+7", b"(a|b){2}7",
    b"(a.){2,}", b"(a|7){1,3}=", b"(?:a|b)=", b"(?:ab){2}", b"(ab?|7=)a", b"(a?|b)7", b"(a*b?)7", b"^(a|b)$", b"^(ab|7)+$", b"^(a|b)",
    b"(7|=)$", b"(a+b)*7", b"(a|b)(7|=)", b"((a))", b"(a|b)+[7=]", b"(\\s|=)(a|A)", b"(a.|b)7", b"([ab]|7){2}=", b"(a|bb|777)=",
    b"(ab|b7){2,4}=", b"(\\x00|a)b", b"(a|\\x80)+7", b"a(b|7)?=", b"(a|b){0,2}7$", b"(?:(?:a|b)(?:7|=)){2}", b"(a|b)*=7", b"((a|b)+7)+=",
    b"(a{2}|b{2})7", b".{0,60}(a|b)7", b"([ab].|7.){2,4}[^=]([aA]|.=)", b"^(\\n|a)*7", b"(A|b)(a|B)",
]
ALL_TRUE_GROUPED = [b"(a|b)*", b"(ab)?", b"(a?|b)", b"(a|7)*$"]


def test_constants():
    assert (_lib.RX_GROUPS, _lib.RX_MAX_EDGES) == (16, 8)
    text = open(os.path.join(ROOT, "include", "kmpgpu.h")).read()
    for name, value in (("KMPGPU_RX_GROUPS", "16u"), ("KMPGPU_RX_MAX_EDGES", "8")):
        assert any(line.split()[:3] == ["#define", name, value] for line in text.splitlines()), name
    assert f"#define KMP_RXG_TILE {_lib.RXG_TILE}u" in open(os.path.join(CSRC, "kmp_regex.h")).read()
    assert "#define KMP_RX_GROUPS 16u" in open(os.path.join(ROOT, "include", "kmphost.h")).read()


def test_grouped_compiler_interpreter_and_packers_under_sanitizers(tmp_path):
    """the model's verdicts first -- none of the expressions is trivially all-true or all-false on these texts, but the ones named as
    such -- then the driver, which must give the model's verdict on every (expression, flags, rule, text), and the linear interpreter's
    for the expressions of tests/test_regex_host.py"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    texts = _texts()
    lines = ["S " + (t.hex() or "-") for t in texts]
    n_expr = n_lin = 0
    assert len(GROUPED) >= 40
    for expr in GROUPED + ALL_TRUE_GROUPED + ACCEPTED + ALL_TRUE:
        for flags in range(4):
            nocase, dotall = bool(flags & RM.NOCASE), bool(flags & RM.DOTALL)
            lines.append(f"X {flags} {expr.hex()}")
            both = []
            for whole in (False, True):
                v = [RM.search(expr, t, nocase, dotall, whole) for t in texts]
                both += v
                lines.append(f"V {int(whole)} " + "".join("01"[x] for x in v))
            if expr in ALL_TRUE or expr in ALL_TRUE_GROUPED:
                assert all(both), expr
            else:
                assert any(both) and not all(both), (expr, flags)
            n_expr += 1
            n_lin += expr in ACCEPTED or expr in ALL_TRUE
    verdicts = tmp_path / "verdicts.txt"
    verdicts.write_text("\n".join(lines) + "\n")

    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    exe = str(tmp_path / "regex_groups_driver")
    subprocess.run(["g++", "-std=c++17", *san, *inc, os.path.join(ROOT, "tests", "regex_groups_sanitizer_driver.cpp"),
                    os.path.join(CSRC, "kmp_regex.cpp"), os.path.join(CSRC, "kmp_rowtables.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, str(verdicts)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "regex groups driver ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert f"{n_expr} expressions, {n_lin} of them linear too, {len(texts)} texts, {n_expr * 2 * len(texts)} verdicts" in r.stdout
