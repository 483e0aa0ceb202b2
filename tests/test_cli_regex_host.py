"""The host side of the expression files: kmp_regexes_parse and the x<q> terms of kmp_rules_parse_rx (include/kmphost.h), and
KMPGPU_REGEX_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options): every refusal, message by
message, on a machine without a GPU -- from the programs exit code 1, nothing on stdout, the message on stderr to the byte -- and a
consistent run, which passes the stage and only then looks for a device.  Without the variable the rules file's messages are what they
were."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DATA, GOLDEN

import regex_model as RM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.host import KmpHostError, parse_regexes

PROGS = [("serial", []), ("openmp_data", ["2"])]
ENOENT = "No such file or directory"
NOT = _lib.RULE_NOT
EIO, EINVAL = -1, -4                                   # KMPHOST_EIO, KMPHOST_EINVAL
FORM = "/EXPR/[i][s] [with <pattern index>]"

TOGETHER = "KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE go together: {} is not set\n"
WITH_RULES = "KMPGPU_REGEX_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE: {} is not set\n"


# ------------------------------------------------------------------------------------------------
# the expressions file
# ------------------------------------------------------------------------------------------------
def _regexes(tmp_path, text, n_pat=3):
    path = tmp_path / "regex.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Regexes()
    err = C.create_string_buffer(_lib.KMP_REGEXES_ERRBUF)
    rc = L.kmp_regexes_parse(str(path).encode(), n_pat, C.byref(r), err)
    if rc:
        assert r.n == 0 and not r.expr and not r.len and not r.flags and not r.gate and not r.bytes and not r.off
        return rc, None, err.value.decode()
    try:
        return 0, [(C.string_at(r.expr[q], r.len[q]), r.flags[q], r.gate[q]) for q in range(r.n)], err.value.decode()
    finally:
        L.kmp_regexes_free(C.byref(r))


def test_an_expressions_file(tmp_path):
    text = (b"# HTTP\n"
            b"/User-Agent: [^\\n]{40,}/\n"
            b"\n"
            b"  /\\d{8,}/i\r\n"
            b"/a.b/s \n"
            b"/= ?x/is with 1\n"
            b"/http://[a-z]+/ with 2\n"
            b"/a b /si\twith  0\n"
            b"\t/\x80\xff+$/\n"
            b"///\n")
    rc, got, msg = _regexes(tmp_path, text)
    assert rc == 0 and msg == ""
    assert got == [(b"User-Agent: [^\\n]{40,}", 0, 0), (b"\\d{8,}", RM.NOCASE, 0), (b"a.b", RM.DOTALL, 0), (b"= ?x", RM.NOCASE | RM.DOTALL | RM.GATED, 1),
                   (b"http://[a-z]+", RM.GATED, 2), (b"a b ", RM.NOCASE | RM.DOTALL | RM.GATED, 0), (b"\x80\xff+$", 0, 0), (b"/", 0, 0)]
    # the Python view of the same file: what GpuMatcher.set_regexes takes
    assert parse_regexes(str(tmp_path / "regex.txt"), 3) == [
        (b"User-Agent: [^\\n]{40,}", {}), (b"\\d{8,}", {"nocase": True}), (b"a.b", {"dotall": True}), (b"= ?x", {"nocase": True, "dotall": True, "gate": 1}),
        (b"http://[a-z]+", {"gate": 2}), (b"a b ", {"nocase": True, "dotall": True, "gate": 0}), (b"\x80\xff+$", {}), (b"/", {})]
    # a file of comments and blank lines holds no expression
    assert _regexes(tmp_path, b"# nothing\n\n   \n")[1] == []
    # more lines than the first allocation holds
    rc, got, msg = _regexes(tmp_path, b"".join(b"/a{%d}/\n" % (i + 1) for i in range(150)))
    assert rc == 0 and len(got) == 150 and got[149] == (b"a{150}", 0, 0)        # (the dialect is kmpgpu_set_regexes' to check)


@pytest.mark.parametrize("text, line, what", [
    (b"abc\n", 1, f"an expression line is {FORM}: it starts with '/'"),
    (b"/ok/\nwith 1\n", 2, "it starts with '/'"),
    (b"/abc\n", 1, f"no closing '/': an expression line is {FORM}"),
    (b"# c\n\n/\n", 3, "no closing '/'"),
    (b"//\n", 1, "an empty expression"),
    (b"//i with 0\n", 1, "an empty expression"),
    (b"/a/x\n", 1, "'x' is not a flag (i: nocase, s: dotall)"),
    (b"/a/I\n", 1, "'I' is not a flag"),
    (b"/a/ii\n", 1, "flag 'i' twice"),
    (b"/a/sis\n", 1, "flag 's' twice"),
    (b"/a/ i\n", 1, "'i' is not 'with <pattern index>'"),
    (b"/a/ after 1\n", 1, "'after' is not 'with <pattern index>'"),
    (b"/a/i with\n", 1, "'with' without a pattern index"),
    (b"/a/ with x\n", 1, "'x' is not a pattern index"),
    (b"/a/ with -1\n", 1, "'-1' is not a pattern index"),
    (b"/a/ with 1x\n", 1, "'1x' is not a pattern index"),
    (b"/a/ with 3\n", 1, "pattern index 3, but there are 3 patterns"),
    (b"/a/ with 99999999999999999999\n", 1, "but there are 3 patterns"),
    (b"/a/ with 1 2\n", 1, "'2' behind the pattern index"),
    (b"/a/\n/b/\n/c/q\n", 3, "'q' is not a flag"),
])
def test_refused_expressions_files(tmp_path, text, line, what):
    rc, got, msg = _regexes(tmp_path, text)
    assert rc == EINVAL and got is None
    assert msg.startswith(f"line {line}: ") and what in msg, msg


def test_missing_expressions_file(tmp_path):
    L = _lib.host_lib()
    r = _lib.Regexes()
    err = C.create_string_buffer(_lib.KMP_REGEXES_ERRBUF)
    assert L.kmp_regexes_parse(str(tmp_path / "nope.txt").encode(), 3, C.byref(r), err) == EIO
    assert "nope.txt" in err.value.decode() and r.n == 0 and not r.expr
    L.kmp_regexes_free(C.byref(r))                        # twice, and NULL
    L.kmp_regexes_free(None)
    with pytest.raises(KmpHostError, match="nope.txt"):
        parse_regexes(str(tmp_path / "nope.txt"), 3)


# ------------------------------------------------------------------------------------------------
# x<q> terms
# ------------------------------------------------------------------------------------------------
def _rules(tmp_path, text, n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx, how="rx"):
    path = tmp_path / "rules.txt"
    path.write_bytes(text)
    L = _lib.host_lib()
    r = _lib.Rules()
    err = C.create_string_buffer(_lib.KMP_RULES_ERRBUF)
    p = str(path).encode()
    if how == "rx":
        rc = L.kmp_rules_parse_rx(p, n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx, C.byref(r), err)
    elif how == "bt":
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


def test_rules_with_expression_terms(tmp_path):
    # 8 patterns, 2 relations, 1 chain, 4 predicates, 3 byte tests, 2 expressions: rows 0..7, 8..9, 10, 11..14, 15..17, 18..19
    text = b"# all six kinds\n0 x0\n\n!x1 2 r1 c0 h3 b2\r\nx1 !x1 x001\n  !7 \t!x0\n"
    rc, rules, msg = _rules(tmp_path, text, 8, 2, 1, 4, 3, 2)
    assert rc == 0 and msg == ""
    assert rules == [[0, 18], [NOT | 19, 2, 9, 10, 14, 17], [19, NOT | 19, 19], [NOT | 7, NOT | 18]]
    # with nothing else set the expressions' rows follow the patterns'
    assert _rules(tmp_path, b"x0 !x1 1\n", 3, 0, 0, 0, 0, 2)[1] == [[3, NOT | 4, 1]]


@pytest.mark.parametrize("text, line, what", [
    (b"0 x2\n", 1, "expression index 2, but there are 2 expressions"),
    (b"0\n!x99999999999\n", 2, "expression index 99999999999"),
    (b"x\n", 1, "'x' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index> or x<expression index>"),
    (b"!x\n", 1, "'!x' is not a pattern index"),
    (b"x1y\n", 1, "'x1y' is not a pattern index"),
    (b"xx1\n", 1, "'xx1' is not a pattern index"),
])
def test_refused_expression_terms(tmp_path, text, line, what):
    rc, rules, msg = _rules(tmp_path, text, 8, 2, 1, 4, 3, 2)
    assert rc == EINVAL and rules is None
    assert msg.startswith(f"line {line}: ") and what in msg, msg


def test_the_old_entries_know_no_expression_terms(tmp_path):
    """kmp_rules_parse, _rel, _terms, _hdr and _bt are kmp_rules_parse_rx with no expressions: "x3" is no term at all, and their messages
    are byte for byte what they were"""
    for how, n_rel, n_chains, n_hdr, n_bt, tail in (
            ("plain", 0, 0, 0, 0, ""), ("rel", 2, 0, 0, 0, " or r<relation index>"), ("terms", 2, 1, 0, 0, " or r<relation index> or c<chain index>"),
            ("hdr", 2, 1, 4, 0, " or r<relation index> or c<chain index> or h<header index>"),
            ("bt", 2, 1, 4, 3, " or r<relation index> or c<chain index> or h<header index> or b<byte test index>")):
        rc, rules, msg = _rules(tmp_path, b"0 1\nx3\n", 8, n_rel, n_chains, n_hdr, n_bt, 0, how)
        assert rc == EINVAL and msg == "line 2: 'x3' is not a pattern index" + tail, msg
    rc, rules, msg = _rules(tmp_path, b"0 x3\n", 8, 2, 1, 4, 3, 0)
    assert rc == EINVAL and msg == "line 1: 'x3' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index>"
    assert _rules(tmp_path, b"!\n", 8, 0, 0, 0, 0, 2)[2] == "line 1: '!' without a pattern index"
    assert _rules(tmp_path, b"0 r1 c0 h2 b1\n", 8, 2, 1, 4, 3, 0, "bt")[1] == [[0, 9, 10, 13, 16]]
    assert _rules(tmp_path, b"9\n", 8, 0, 0, 0, 0, 2)[2] == "line 1: pattern index 9, but there are 8 patterns"
    assert _rules(tmp_path, b"b3\n", 8, 0, 0, 0, 3, 2)[2] == "line 1: byte test index 3, but there are 3 byte tests"


def test_too_many_rows_for_a_term(tmp_path):
    rc, rules, msg = _rules(tmp_path, b"0\n", (1 << 31) - 8, 1, 1, 2, 2, 2)
    assert rc == EINVAL and "line" not in msg
    assert msg == "2147483640 patterns + 1 relations + 1 chains + 2 header predicates + 2 byte tests + 2 expressions do not fit the 2^31 rows a term can name"
    assert _rules(tmp_path, b"0 x1\n", (1 << 31) - 9, 1, 1, 2, 2, 2)[1] == [[0, (1 << 31) - 2]]
    # without expressions the message is the byte tests' own
    rc, rules, msg = _rules(tmp_path, b"0\n", (1 << 31) - 6, 1, 1, 2, 2, 0)
    assert rc == EINVAL and msg == "2147483642 patterns + 1 relations + 1 chains + 2 header predicates + 2 byte tests do not fit the 2^31 rows a term can name"


# ------------------------------------------------------------------------------------------------
# the programs' options stage
# ------------------------------------------------------------------------------------------------
def run(prog, extra, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("KMPGPU_")}
    env.update({"KMPGPU_" + k: str(v) for k, v in env_extra.items()})
    return subprocess.run([os.path.join(_lib.BINDIR, prog), os.path.join(DATA, "udp_1000.pcap"), os.path.join(DATA, "strings.txt"), *extra, "udp"],
                          capture_output=True, text=True, timeout=120, env=env)


def refused(prog, extra, env_extra, message):
    r = run(prog, extra, env_extra)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", message), env_extra


@pytest.fixture
def files(tmp_path):
    text = {"rules": "0 !1 x0\nr0 c0 h0 b0 !x1\n", "plain_rules": "0 !1\n2\n", "relations": "0 1 * 40\n", "chains": "0 0 * 1 -3 9 2\n",
            "headers": "udp any any -> any 53\n", "windows": "0 0 63\n", "bytetests": "2 & 0x8000 2\n",
            "regex": "# /EXPR/[i][s] [with <pattern index>]\n/[a-z]{4,}\\.com/i\n/\\d+$/ with 1\n"}
    out = {}
    for name, body in text.items():
        out[name] = tmp_path / (name + ".txt")
        out[name].write_text(body)
    out["alerts"] = tmp_path / "alerts.csv"
    out["flow_alerts"] = tmp_path / "flow_alerts.csv"
    out["export"] = tmp_path / "export.pcap"
    out["missing"] = tmp_path / "no_such_file.txt"
    return out


@pytest.mark.parametrize("prog,extra", PROGS)
def test_expressions_file_goes_with_rules_and_an_alerts_file(files, prog, extra):
    f = files
    own = {"REGEX_FILE": f["regex"]}
    refused(prog, extra, own, WITH_RULES.format("KMPGPU_RULES_FILE"))
    refused(prog, extra, dict(own, ALERTS_FILE=f["alerts"]), TOGETHER.format("KMPGPU_RULES_FILE"))
    # with rules but no alerts file: the pair's own refusal comes first; an export lifts that one, not the expressions'
    refused(prog, extra, dict(own, RULES_FILE=f["plain_rules"]), TOGETHER.format("KMPGPU_ALERTS_FILE"))
    refused(prog, extra, dict(own, RULES_FILE=f["plain_rules"], EXPORT_FILE=f["export"]), WITH_RULES.format("neither of the two"))
    # an empty value is no value: the variable is not set, and the rules' x0 is no term
    refused(prog, extra, {"REGEX_FILE": "", "RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"]},
            f"error reading rules file {f['rules']}: line 1: 'x0' is not a pattern index\n")
    assert not f["alerts"].exists() and not f["flow_alerts"].exists()


BAD = [("/ok/\nnope\n", "line 2: an expression line is " + FORM + ": it starts with '/'"),
       ("# c\n/abc\n", "line 2: no closing '/': an expression line is " + FORM),
       ("\n//\n", "line 2: an empty expression"),
       ("/a/g\n", "line 1: 'g' is not a flag (i: nocase, s: dotall)"),
       ("/a/ss\n", "line 1: flag 's' twice"),
       ("/a/ gate 1\n", "line 1: 'gate' is not 'with <pattern index>'"),
       ("/a/ with\n", "line 1: 'with' without a pattern index"),
       ("/a/ with 9999\n", "line 1: pattern index 9999, but there are {n} patterns"),
       ("/a/ with 1 i\n", "line 1: 'i' behind the pattern index")]


@pytest.mark.parametrize("prog,extra", PROGS)
def test_expressions_files_that_do_not_parse_or_do_not_exist(files, tmp_path, tokens, prog, extra):
    f = files
    both = {"RULES_FILE": f["plain_rules"], "ALERTS_FILE": f["alerts"]}
    bad = tmp_path / "bad.txt"
    for text, message in BAD:
        bad.write_text(text)
        refused(prog, extra, dict(both, REGEX_FILE=bad), f"error reading expressions file {bad}: {message.format(n=len(tokens))}\n")
    refused(prog, extra, dict(both, REGEX_FILE=f["missing"]), f"error reading expressions file {f['missing']}: {f['missing']}: {ENOENT}\n")
    # an index beyond the file's lines is refused with the rules file's line
    every = dict(both, RULES_FILE=f["rules"], RELATIONS_FILE=f["relations"], CHAINS_FILE=f["chains"], HEADERS_FILE=f["headers"],
                 BYTETESTS_FILE=f["bytetests"])
    one = tmp_path / "one.txt"
    one.write_text("/abc/\n")
    refused(prog, extra, dict(every, REGEX_FILE=one), f"error reading rules file {f['rules']}: line 2: expression index 1, but there are 1 expressions\n")
    # the byte tests are read before the expressions, the expressions before the rules, the windows last
    bad.write_text("nothing\n")
    wrong = dict(every, BYTETESTS_FILE=bad, REGEX_FILE=bad, RULES_FILE=bad, WINDOWS_FILE=bad)
    refused(prog, extra, wrong,
            f"error reading byte tests file {bad}: line 1: 1 of the four fields that begin <nbytes> <op> <value> <offset> [after <pattern index>] [little] [mask <m>]\n")
    refused(prog, extra, dict(wrong, BYTETESTS_FILE=f["bytetests"]),
            f"error reading expressions file {bad}: line 1: an expression line is {FORM}: it starts with '/'\n")
    refused(prog, extra, dict(wrong, BYTETESTS_FILE=f["bytetests"], REGEX_FILE=f["regex"]),
            f"error reading rules file {bad}: line 1: 'nothing' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index> or x<expression index>\n")
    refused(prog, extra, dict(wrong, BYTETESTS_FILE=f["bytetests"], REGEX_FILE=f["regex"], RULES_FILE=f["rules"]),
            f"error reading windows file {bad}: line 1: 'nothing' is not a pattern index\n")
    assert not f["alerts"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_rules_file_messages_are_unchanged_without_an_expressions_file(files, tmp_path, prog, extra):
    """no KMPGPU_REGEX_FILE: "x<q>" is no term, and every message of the rules file is byte for byte what it was"""
    f = files
    both = {"ALERTS_FILE": f["alerts"]}
    rules = tmp_path / "r.txt"
    rules.write_text("0 1\nx0\n")
    refused(prog, extra, dict(both, RULES_FILE=rules), f"error reading rules file {rules}: line 2: 'x0' is not a pattern index\n")
    refused(prog, extra, dict(both, RULES_FILE=rules, RELATIONS_FILE=f["relations"]),
            f"error reading rules file {rules}: line 2: 'x0' is not a pattern index or r<relation index>\n")
    refused(prog, extra, dict(both, RULES_FILE=rules, RELATIONS_FILE=f["relations"], CHAINS_FILE=f["chains"], HEADERS_FILE=f["headers"],
                              BYTETESTS_FILE=f["bytetests"]),
            f"error reading rules file {rules}: line 2: 'x0' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index>\n")
    rules.write_text("0 !\n")
    refused(prog, extra, dict(both, RULES_FILE=rules), f"error reading rules file {rules}: line 1: '!' without a pattern index\n")
    rules.write_text("0 b1\n")
    refused(prog, extra, dict(both, RULES_FILE=rules, BYTETESTS_FILE=f["bytetests"]),
            f"error reading rules file {rules}: line 1: byte test index 1, but there are 1 byte tests\n")
    assert not f["alerts"].exists()


def test_flow_alerts_file_serves_in_the_alerts_file_s_place(files):
    """with KMPGPU_FLOW_ALERTS_FILE the expressions need no KMPGPU_ALERTS_FILE; more than one shard is the flows' own refusal"""
    f = files
    env = {"REGEX_FILE": f["regex"], "RULES_FILE": f["plain_rules"], "FLOW_ALERTS_FILE": f["flow_alerts"]}
    refused("openmp_data", ["2"], env,
            "KMPGPU_FLOWS_FILE and KMPGPU_FLOW_ALERTS_FILE need one shard, thread_number is 2: a flow would be cut at a shard's edge\n")
    bad = files["missing"]
    refused("serial", [], dict(env, REGEX_FILE=bad), f"error reading expressions file {bad}: {bad}: {ENOENT}\n")


def test_openmp_task_ignores_the_variable(files):
    """bin/openmp_task has no rules: KMPGPU_REGEX_FILE is not read there, whatever it names"""
    r = subprocess.run([os.path.join(_lib.BINDIR, "openmp_task"), os.path.join(DATA, "udp_1000.pcap"), os.path.join(DATA, "strings.txt"), "2", "udp"],
                       capture_output=True, text=True, timeout=120,
                       env=dict({k: v for k, v in os.environ.items() if not k.startswith("KMPGPU_")}, KMPGPU_REGEX_FILE=str(files["missing"])))
    assert "expressions file" not in r.stderr and "KMPGPU_REGEX_FILE" not in r.stderr


@pytest.mark.parametrize("env_name", ["ALERTS_FILE", "FLOW_ALERTS_FILE"])
def test_expressions_file_passes_the_options_stage(files, env_name):
    """... and ends where a plain run ends: without a device with exit code 2 and the device message, with one with the golden counts"""
    import torch
    f = files
    out = f["alerts"] if env_name == "ALERTS_FILE" else f["flow_alerts"]
    env = {"RULES_FILE": f["rules"], env_name: out, "REGEX_FILE": f["regex"]}
    if env_name == "ALERTS_FILE":                          # (the relations, chains and headers files ask for KMPGPU_ALERTS_FILE themselves)
        env.update({"RELATIONS_FILE": f["relations"], "CHAINS_FILE": f["chains"], "HEADERS_FILE": f["headers"], "BYTETESTS_FILE": f["bytetests"]})
    else:
        f["rules"].write_text("0 !1 x0\n!x1\n")
    r = run("serial", [], env)
    if torch.cuda.is_available():
        with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as g:
            golden = g.read()
        assert r.returncode == 0 and r.stdout.startswith(golden) and out.exists(), r.stderr
    else:
        assert (r.returncode, r.stdout) == (2, "") and r.stderr.startswith("no MI355X device: ") and r.stderr.count("\n") == 1, r.stderr
        assert not f["alerts"].exists()
