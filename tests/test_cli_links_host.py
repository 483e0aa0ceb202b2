"""KMPGPU_LINKS_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options) on a machine without a
GPU: every refusal it makes before any GPU work, with exit code 1, nothing on stdout and the message on stderr to the byte.
bin/openmp_task ignores the variable."""
import os
import subprocess

import pytest

from conftest import DATA

from multithreading_string_matching_amd import _lib

PROGS = [("serial", []), ("openmp_data", ["1"])]
WITH = "KMPGPU_LINKS_FILE does not go together with KMPGPU_"
ONE = "there the rows come from one buffer; a line '{}' links it\n"
NOT_WITH = {
    ("DECODE", "percent"): WITH + "DECODE: " + ONE.format("decode:percent <term>"),
    ("HTTP_FIELD", "body"): WITH + "HTTP_FIELD: " + ONE.format("http:<field> <term>"),
    ("DNS_FIELD", "qname"): WITH + "DNS_FIELD: " + ONE.format("dns:qname <term>"),
    ("BASE64", "16"): WITH + "BASE64: " + ONE.format("base64:<min_run> <term>"),
    ("FLOW_SEAMS", "32"): WITH + "FLOW_SEAMS: seams are numbered by themselves, links in this program by the capture's payloads\n",
    ("FLOW_STREAMS", "1m"): WITH + "FLOW_STREAMS: streams are numbered by themselves, links in this program by the capture's payloads\n",
}
NO_RULES = "KMPGPU_LINKS_FILE goes together with KMPGPU_RULES_FILE: a link is a term l<q> of a rule\n"
BUFFERS = "(http:method|raw_uri|uri|status|headers|body, dns:qname[,tcp], decode:percent[+plus], base64:<min_run>[,url])"
N_PAT = 97                                # tokens of strings.txt


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
    out = {"links": tmp_path / "links.txt", "rules": tmp_path / "rules.txt", "alerts": tmp_path / "alerts.csv", "relations": tmp_path / "relations.txt"}
    out["links"].write_text("# two buffers\nhttp:uri 3\n\nhttp:body 7\n")
    out["rules"].write_text("l0 l1\n0 !l1\n")
    out["relations"].write_text("0 1 0 10\n")
    return out


def base(f, **more):
    return dict({"LINKS_FILE": f["links"], "RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"]}, **more)


@pytest.mark.parametrize("prog,extra", PROGS)
def test_variables_it_does_not_go_with(files, prog, extra):
    for (var, value), message in NOT_WITH.items():
        refused(prog, extra, base(files, **{var: value}), message)
    refused(prog, extra, {"LINKS_FILE": files["links"]}, NO_RULES)


@pytest.mark.parametrize("prog,extra", PROGS)
def test_links_files_that_are_refused(files, prog, extra):
    f = files
    path = str(f["links"])
    head = f"error reading links file {path}: "
    cases = [
        ("http:body !3\n", head + "line 1: a link's term is not negated: the rule that names the link negates it\n"),
        ("http:body 3\nhttp:uri l0\n", head + "line 2: a link's term names no link\n"),
        (f"http:body {N_PAT}\n", head + f"line 1: pattern index {N_PAT}, but there are {N_PAT} patterns\n"),
        ("http:body r0\n", head + "line 1: 'r0' is not a pattern index\n"),                       # no relations: the token is no term
        ("http:body\n", head + "line 1: 'http:body' without a term: a line is <buffer> <term>\n"),
        ("http:body 1 2\n", head + "line 1: 2 terms: a link is one term\n"),
        ("x" * 64 + " 1\n", head + "line 1: a buffer word of 64 characters: at most 63\n"),
        ("http:cookie 1\n", f"KMPGPU_LINKS_FILE: link 0: 'http:cookie' is no buffer {BUFFERS}\n"),
        ("http:body 1\ntls:sni 2\n", f"KMPGPU_LINKS_FILE: link 1: 'tls:sni' is no buffer {BUFFERS}\n"),
        ("body 1\n", f"KMPGPU_LINKS_FILE: link 0: 'body' is no buffer {BUFFERS}\n"),
        ("base64:3 1\n", f"KMPGPU_LINKS_FILE: link 0: 'base64:3' is no buffer {BUFFERS}\n"),
        ("dns:qname,udp 1\n", f"KMPGPU_LINKS_FILE: link 0: 'dns:qname,udp' is no buffer {BUFFERS}\n"),
    ]
    for text, message in cases:
        f["links"].write_text(text)
        refused(prog, extra, base(f), message)
    # with relations the same r-token is a term, and one out of range is named as such
    f["links"].write_text("http:body r1\n")
    refused(prog, extra, base(f, RELATIONS_FILE=f["relations"]), head + "line 1: relation index 1, but there are 1 relations\n")
    # nine distinct buffers; the same buffer twice is one
    nine = ["http:method", "http:raw_uri", "http:uri", "http:status", "http:headers", "http:body", "dns:qname", "dns:qname,tcp", "decode:percent"]
    f["links"].write_text("".join(f"{b} 1\n" for b in nine[:8] + nine[:8] + nine[8:]))
    refused(prog, extra, base(f), "KMPGPU_LINKS_FILE: link 16: 'decode:percent' is buffer 9: at most 8 distinct buffers\n")
    refused(prog, extra, base(f, LINKS_FILE="/no/such/dir/links.txt"), "error reading links file /no/such/dir/links.txt: /no/such/dir/links.txt: No such file or directory\n")


@pytest.mark.parametrize("prog,extra", PROGS)
def test_rules_files_with_link_terms(files, prog, extra):
    f = files
    head = f"error reading rules file {f['rules']}: "
    f["rules"].write_text("l0 !l2\n")
    refused(prog, extra, base(f), head + "line 1: link index 2, but there are 2 links\n")
    f["rules"].write_text("0 lx\n")
    refused(prog, extra, base(f), head + "line 1: 'lx' is not a pattern index or l<link index>\n")
    # without the links file the letter is no term at all
    f["rules"].write_text("l0\n")
    refused(prog, extra, {"RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"]}, head + "line 1: 'l0' is not a pattern index\n")


@pytest.mark.parametrize("prog,extra", PROGS)
def test_a_consistent_setting_passes_the_stage(files, prog, extra):
    """... and only then looks for a device: whatever ends the run then, it is none of the stage's messages"""
    r = run(prog, extra, base(files))
    assert "KMPGPU_LINKS_FILE" not in r.stderr and "error reading" not in r.stderr, r.stderr
    assert r.returncode in (0, 2), (r.returncode, r.stderr)


def test_openmp_task_ignores_the_variable(files):
    r = run("openmp_task", ["1"], {"LINKS_FILE": files["links"]})
    assert "KMPGPU_LINKS_FILE" not in r.stderr and r.returncode != 1, (r.returncode, r.stderr)
