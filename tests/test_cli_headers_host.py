"""KMPGPU_HEADERS_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options): every refusal the
programs make for it, on a machine without a GPU -- exit code 1, nothing on stdout, the message on stderr to the byte -- and a consistent
run, which passes the stage and only then looks for a device.  The variable is accepted and refused as KMPGPU_CHAINS_FILE is."""
import os
import subprocess

import pytest

from conftest import DATA, GOLDEN

from multithreading_string_matching_amd import _lib

PROGS = [("serial", []), ("openmp_data", ["2"])]
ENOENT = "No such file or directory"

TOGETHER = "KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE go together: {} is not set\n"
WITH_BOTH = "KMPGPU_HEADERS_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: {} is not set\n"


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
    text = {"rules": "0 !1 h0\nr0 c0 !h1\n", "plain_rules": "0 !1\n2\n", "relations": "0 1 * 40\n", "chains": "0 0 * 1 -3 9 2\n",
            "headers": "# proto src sport dir dst dport [len]\nudp 10.0.0.0/8 any -> any 53\nany any any <> any 1024: 1:\n", "windows": "0 0 63\n"}
    out = {}
    for name, body in text.items():
        out[name] = tmp_path / (name + ".txt")
        out[name].write_text(body)
    out["alerts"] = tmp_path / "alerts.csv"
    out["export"] = tmp_path / "export.pcap"
    out["missing"] = tmp_path / "no_such_file.txt"
    return out


@pytest.mark.parametrize("prog,extra", PROGS)
def test_headers_file_goes_with_rules_and_alerts(files, prog, extra):
    f = files
    own = {"HEADERS_FILE": f["headers"]}
    refused(prog, extra, own, WITH_BOTH.format("KMPGPU_RULES_FILE"))
    refused(prog, extra, dict(own, ALERTS_FILE=f["alerts"]), TOGETHER.format("KMPGPU_RULES_FILE"))
    # with rules but no alerts file: the pair's own refusal comes first; an export lifts that one, not the headers'
    refused(prog, extra, dict(own, RULES_FILE=f["plain_rules"]), TOGETHER.format("KMPGPU_ALERTS_FILE"))
    refused(prog, extra, dict(own, RULES_FILE=f["plain_rules"], EXPORT_FILE=f["export"]), WITH_BOTH.format("KMPGPU_ALERTS_FILE"))
    # an empty value is no value: the variable is not set, and the rules' h0 is no term
    refused(prog, extra, {"HEADERS_FILE": "", "RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"]},
            f"error reading rules file {f['rules']}: line 1: 'h0' is not a pattern index\n")
    assert not f["alerts"].exists()


BAD = [("udp any any -> any 53\nudp any any -> any\n", "line 2: 5 of the six or seven fields <proto> <src> <sport> <dir> <dst> <dport> [<len>]"),
       ("# c\nicmp any any -> any any\n", "line 2: 'icmp' is not a protocol (udp, tcp, ip, any or 0..255)"),
       ("\nudp 10.0.0.0/33 any -> any any\n", "line 2: '10.0.0.0/33' is not an address (any, a.b.c.d or a.b.c.d/0..32)"),
       ("ip any any -> any any\nudp any 9:8 -> any any\n", "line 2: '9:8': port 9 lies above 8"),
       ("ip any any -> any any\nudp any any >> any any\n", "line 2: '>>' is not a direction (-> or <>)"),
       ("ip any any -> any any\nudp any any -> any any 5:4\n", "line 2: '5:4': length 5 lies above 4")]


@pytest.mark.parametrize("prog,extra", PROGS)
def test_headers_files_that_do_not_parse_or_do_not_exist(files, tmp_path, prog, extra):
    f = files
    both = {"RULES_FILE": f["plain_rules"], "ALERTS_FILE": f["alerts"]}
    bad = tmp_path / "bad.txt"
    for text, message in BAD:
        bad.write_text(text)
        refused(prog, extra, dict(both, HEADERS_FILE=bad), f"error reading headers file {bad}: {message}\n")
    refused(prog, extra, dict(both, HEADERS_FILE=f["missing"]), f"error reading headers file {f['missing']}: {f['missing']}: {ENOENT}\n")
    # h0 is a term only where the headers file is there, and an index beyond its lines is refused with the rules file's line
    every = dict(both, RULES_FILE=f["rules"], RELATIONS_FILE=f["relations"], CHAINS_FILE=f["chains"])
    refused(prog, extra, every, f"error reading rules file {f['rules']}: line 1: 'h0' is not a pattern index or r<relation index> or c<chain index>\n")
    few = tmp_path / "few.txt"
    few.write_text("ip any any -> any any\n")
    refused(prog, extra, dict(every, HEADERS_FILE=few), f"error reading rules file {f['rules']}: line 2: header index 1, but there are 1 header predicates\n")
    # the chains are read before the headers, the headers before the rules, the windows last
    bad.write_text("nothing\n")
    wrong = dict(every, CHAINS_FILE=bad, HEADERS_FILE=bad, RULES_FILE=bad, WINDOWS_FILE=bad)
    refused(prog, extra, wrong, f"error reading chains file {bad}: line 1: 'nothing' is not a pattern index\n")
    refused(prog, extra, dict(wrong, CHAINS_FILE=f["chains"]),
            f"error reading headers file {bad}: line 1: 1 of the six or seven fields <proto> <src> <sport> <dir> <dst> <dport> [<len>]\n")
    refused(prog, extra, dict(wrong, CHAINS_FILE=f["chains"], HEADERS_FILE=f["headers"]),
            f"error reading rules file {bad}: line 1: 'nothing' is not a pattern index or r<relation index> or c<chain index> or h<header index>\n")
    refused(prog, extra, dict(wrong, CHAINS_FILE=f["chains"], HEADERS_FILE=f["headers"], RULES_FILE=f["rules"]),
            f"error reading windows file {bad}: line 1: 'nothing' is not a pattern index\n")
    assert not f["alerts"].exists()


@pytest.mark.parametrize("device_extract", ["0", "1"])
@pytest.mark.parametrize("prog,extra", PROGS)
def test_headers_file_passes_the_options_stage(files, prog, extra, device_extract):
    """... and ends where a plain run ends: without a device with exit code 2 and the device message, with one with the golden counts"""
    import torch
    f = files
    r = run(prog, extra, {"RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"], "RELATIONS_FILE": f["relations"], "CHAINS_FILE": f["chains"],
                          "HEADERS_FILE": f["headers"], "DEVICE_EXTRACT": device_extract})
    if torch.cuda.is_available():
        with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as g:
            golden = g.read()
        assert r.returncode == 0 and r.stdout.startswith(golden) and f["alerts"].exists(), r.stderr
    else:
        assert (r.returncode, r.stdout) == (2, "") and r.stderr.startswith("no MI355X device: ") and r.stderr.count("\n") == 1, r.stderr
        assert not f["alerts"].exists()
