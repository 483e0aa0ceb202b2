"""KMPGPU_BYTETESTS_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options): every refusal the
programs make for it, on a machine without a GPU -- exit code 1, nothing on stdout, the message on stderr to the byte -- and a consistent
run, which passes the stage and only then looks for a device.  Without the variable the rules file's messages are what they were."""
import os
import subprocess

import pytest

from conftest import DATA, GOLDEN

from multithreading_string_matching_amd import _lib

PROGS = [("serial", []), ("openmp_data", ["2"])]
ENOENT = "No such file or directory"

TOGETHER = "KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE go together: {} is not set\n"
WITH_RULES = "KMPGPU_BYTETESTS_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE: {} is not set\n"


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
    text = {"rules": "0 !1 b0\nr0 c0 h0 !b1\n", "plain_rules": "0 !1\n2\n", "relations": "0 1 * 40\n", "chains": "0 0 * 1 -3 9 2\n",
            "headers": "udp any any -> any 53\n", "windows": "0 0 63\n",
            "bytetests": "# nbytes op value offset [after i] [little] [mask m]\n2 & 0x8000 2\n2 > 512 0 after 1 little\n"}
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
def test_byte_tests_file_goes_with_rules_and_an_alerts_file(files, prog, extra):
    f = files
    own = {"BYTETESTS_FILE": f["bytetests"]}
    refused(prog, extra, own, WITH_RULES.format("KMPGPU_RULES_FILE"))
    refused(prog, extra, dict(own, ALERTS_FILE=f["alerts"]), TOGETHER.format("KMPGPU_RULES_FILE"))
    # with rules but no alerts file: the pair's own refusal comes first; an export lifts that one, not the byte tests'
    refused(prog, extra, dict(own, RULES_FILE=f["plain_rules"]), TOGETHER.format("KMPGPU_ALERTS_FILE"))
    refused(prog, extra, dict(own, RULES_FILE=f["plain_rules"], EXPORT_FILE=f["export"]), WITH_RULES.format("neither of the two"))
    # an empty value is no value: the variable is not set, and the rules' b0 is no term
    refused(prog, extra, {"BYTETESTS_FILE": "", "RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"]},
            f"error reading rules file {f['rules']}: line 1: 'b0' is not a pattern index\n")
    assert not f["alerts"].exists() and not f["flow_alerts"].exists()


BAD = [("2 = 1 4\n2 = 1\n", "line 2: 3 of the four fields that begin <nbytes> <op> <value> <offset> [after <pattern index>] [little] [mask <m>]"),
       ("# c\n8 = 1 0\n", "line 2: '8' is not a byte count (1..4)"),
       ("\n2 =< 1 0\n", "line 2: '=<' is not an operator (= != < > <= >= &)"),
       ("2 = 0x1ffffffff 0\n", "line 1: '0x1ffffffff' is not a value (0..4294967295, decimal or 0x hex)"),
       ("2 = 1 -3\n", "line 1: offset -3 lies in front of the payload: only a test after a pattern reaches back"),
       ("2 = 1 0 after 9999\n", "line 1: pattern index 9999, but there are {n} patterns"),
       ("2 & 1 0 mask 3\n", "line 1: '&' takes its mask from <value>: it has no mask clause"),
       ("2 = 1 0 big\n", "line 1: 'big' is none of after <pattern index>, little, mask <m>")]


@pytest.mark.parametrize("prog,extra", PROGS)
def test_byte_tests_files_that_do_not_parse_or_do_not_exist(files, tmp_path, tokens, prog, extra):
    f = files
    both = {"RULES_FILE": f["plain_rules"], "ALERTS_FILE": f["alerts"]}
    bad = tmp_path / "bad.txt"
    for text, message in BAD:
        bad.write_text(text)
        refused(prog, extra, dict(both, BYTETESTS_FILE=bad), f"error reading byte tests file {bad}: {message.format(n=len(tokens))}\n")
    refused(prog, extra, dict(both, BYTETESTS_FILE=f["missing"]), f"error reading byte tests file {f['missing']}: {f['missing']}: {ENOENT}\n")
    # an index beyond the file's lines is refused with the rules file's line
    every = dict(both, RULES_FILE=f["rules"], RELATIONS_FILE=f["relations"], CHAINS_FILE=f["chains"], HEADERS_FILE=f["headers"])
    one = tmp_path / "one.txt"
    one.write_text("1 >= 0 11\n")
    refused(prog, extra, dict(every, BYTETESTS_FILE=one), f"error reading rules file {f['rules']}: line 2: byte test index 1, but there are 1 byte tests\n")
    # the headers are read before the byte tests, the byte tests before the rules, the windows last
    bad.write_text("nothing\n")
    wrong = dict(every, HEADERS_FILE=bad, BYTETESTS_FILE=bad, RULES_FILE=bad, WINDOWS_FILE=bad)
    refused(prog, extra, wrong, f"error reading headers file {bad}: line 1: 1 of the six or seven fields <proto> <src> <sport> <dir> <dst> <dport> [<len>]\n")
    refused(prog, extra, dict(wrong, HEADERS_FILE=f["headers"]),
            f"error reading byte tests file {bad}: line 1: 1 of the four fields that begin <nbytes> <op> <value> <offset> [after <pattern index>] [little] [mask <m>]\n")
    refused(prog, extra, dict(wrong, HEADERS_FILE=f["headers"], BYTETESTS_FILE=f["bytetests"]),
            f"error reading rules file {bad}: line 1: 'nothing' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index>\n")
    refused(prog, extra, dict(wrong, HEADERS_FILE=f["headers"], BYTETESTS_FILE=f["bytetests"], RULES_FILE=f["rules"]),
            f"error reading windows file {bad}: line 1: 'nothing' is not a pattern index\n")
    assert not f["alerts"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_rules_file_messages_are_unchanged_without_a_byte_tests_file(files, tmp_path, prog, extra):
    """no KMPGPU_BYTETESTS_FILE: "b<q>" is no term, and every message of the rules file is byte for byte what it was"""
    f = files
    both = {"ALERTS_FILE": f["alerts"]}
    rules = tmp_path / "r.txt"
    rules.write_text("0 1\nb0\n")
    refused(prog, extra, dict(both, RULES_FILE=rules), f"error reading rules file {rules}: line 2: 'b0' is not a pattern index\n")
    refused(prog, extra, dict(both, RULES_FILE=rules, RELATIONS_FILE=f["relations"]),
            f"error reading rules file {rules}: line 2: 'b0' is not a pattern index or r<relation index>\n")
    refused(prog, extra, dict(both, RULES_FILE=rules, RELATIONS_FILE=f["relations"], CHAINS_FILE=f["chains"], HEADERS_FILE=f["headers"]),
            f"error reading rules file {rules}: line 2: 'b0' is not a pattern index or r<relation index> or c<chain index> or h<header index>\n")
    rules.write_text("0 !\n")
    refused(prog, extra, dict(both, RULES_FILE=rules), f"error reading rules file {rules}: line 1: '!' without a pattern index\n")
    rules.write_text("99999\n")
    r = run(prog, extra, dict(both, RULES_FILE=rules))
    assert (r.returncode, r.stdout) == (1, "") and r.stderr.startswith(f"error reading rules file {rules}: line 1: pattern index 99999, but there are ")
    rules.write_text("0 h1\n")
    refused(prog, extra, dict(both, RULES_FILE=rules, HEADERS_FILE=f["headers"]),
            f"error reading rules file {rules}: line 1: header index 1, but there are 1 header predicates\n")
    assert not f["alerts"].exists()


def test_flow_alerts_file_serves_in_the_alerts_file_s_place(files):
    """with KMPGPU_FLOW_ALERTS_FILE the byte tests need no KMPGPU_ALERTS_FILE; more than one shard is the flows' own refusal"""
    f = files
    env = {"BYTETESTS_FILE": f["bytetests"], "RULES_FILE": f["plain_rules"], "FLOW_ALERTS_FILE": f["flow_alerts"]}
    refused("openmp_data", ["2"], env,
            "KMPGPU_FLOWS_FILE and KMPGPU_FLOW_ALERTS_FILE need one shard, thread_number is 2: a flow would be cut at a shard's edge\n")
    bad = files["missing"]
    refused("serial", [], dict(env, BYTETESTS_FILE=bad), f"error reading byte tests file {bad}: {bad}: {ENOENT}\n")


@pytest.mark.parametrize("env_name", ["ALERTS_FILE", "FLOW_ALERTS_FILE"])
def test_byte_tests_file_passes_the_options_stage(files, env_name):
    """... and ends where a plain run ends: without a device with exit code 2 and the device message, with one with the golden counts"""
    import torch
    f = files
    out = f["alerts"] if env_name == "ALERTS_FILE" else f["flow_alerts"]
    env = {"RULES_FILE": f["rules"], env_name: out, "BYTETESTS_FILE": f["bytetests"]}
    if env_name == "ALERTS_FILE":                          # (the relations, chains and headers files ask for KMPGPU_ALERTS_FILE themselves)
        env.update({"RELATIONS_FILE": f["relations"], "CHAINS_FILE": f["chains"], "HEADERS_FILE": f["headers"]})
    else:
        f["rules"].write_text("0 !1 b0\n!b1\n")
    r = run("serial", [], env)
    if torch.cuda.is_available():
        with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as g:
            golden = g.read()
        assert r.returncode == 0 and r.stdout.startswith(golden) and out.exists(), r.stderr
    else:
        assert (r.returncode, r.stdout) == (2, "") and r.stderr.startswith("no MI355X device: ") and r.stderr.count("\n") == 1, r.stderr
        assert not f["alerts"].exists()
