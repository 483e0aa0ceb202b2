"""KMPGPU_FLOW_SEAMS in bin/serial and bin/openmp_data (csrc/host/kmp_cli.c).  The refusals of the options stage need no GPU: they are made
before any GPU work, with exit code 1, nothing on stdout and the message on stderr to the byte.  On the GPU: a small capture written
here, with one content split across two TCP segments, whose flow alerts differ with and without the variable exactly as
tests/seam_model.py says."""
import os
import subprocess

import numpy as np
import pytest

import flow_model as FM
import header_model as HM
import match_model as MM
import seam_model as SM
from multithreading_string_matching_amd import _lib

from test_cli_flows_host import ONE_SHARD
from test_cli_options_host import refused, run

NEEDS_FLOW_ALERTS = "KMPGPU_FLOW_SEAMS goes together with KMPGPU_FLOW_ALERTS_FILE: it is not set\n"
BAD_REACH = "KMPGPU_FLOW_SEAMS is \"{}\": a reach of 1..98 bytes is needed\n"
PROGS = [("serial", []), ("openmp_data", ["1"])]


@pytest.fixture
def files(tmp_path):
    rules = tmp_path / "rules.txt"
    rules.write_text("0 !1\n2\n")
    return {"rules": rules, "flows": tmp_path / "flows.csv", "flow_alerts": tmp_path / "flow_alerts.csv"}


@pytest.mark.parametrize("prog,extra", PROGS)
def test_seams_need_the_flow_alerts_file_and_a_reach(files, prog, extra):
    f = files
    refused(prog, extra, {"FLOW_SEAMS": "98"}, NEEDS_FLOW_ALERTS)
    refused(prog, extra, {"FLOW_SEAMS": "98", "FLOWS_FILE": f["flows"]}, NEEDS_FLOW_ALERTS)
    good = {"FLOW_ALERTS_FILE": f["flow_alerts"], "RULES_FILE": f["rules"]}
    for reach in ("0", "99", "-1", "x", "16x", " ", "1e1", "98.0", "4294967297"):
        refused(prog, extra, dict(good, FLOW_SEAMS=reach), BAD_REACH.format(reach))


def test_more_than_one_shard(files):
    f = files
    refused("openmp_data", ["2"], {"FLOW_SEAMS": "98", "FLOW_ALERTS_FILE": f["flow_alerts"], "RULES_FILE": f["rules"]}, ONE_SHARD.format("2"))
    assert not f["flow_alerts"].exists()


def test_openmp_task_ignores_the_variable():
    import torch
    r = run("openmp_task", [], {"FLOW_SEAMS": "0"})
    assert "KMPGPU_FLOW" not in r.stderr and r.returncode == (0 if torch.cuda.is_available() else 2), r.stderr


# ------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------
CLIENT, SERVER, OTHER = 0x0A000001, 0xC0A80101, 0x0A000002


def _capture():
    """Ethernet / IPv4 / TCP frames: a client's request in two segments with the server's answer and another connection's segment in
    between, a connection whose split content is barred by a negated one split the same way, and one that holds the content whole."""
    seg = [
        (CLIENT, 40000, SERVER, 80, b"GET /adm"),
        (SERVER, 80, CLIENT, 40000, b"HTTP/1.1 100 Continue\r\n"),
        (OTHER, 40001, SERVER, 80, b"GET /index.html HTTP/1.1\r\n"),
        (CLIENT, 40000, SERVER, 80, b"in HTTP/1.1\r\nHost: example\r\n"),
        (OTHER, 40002, SERVER, 80, b"GET /admin HTTP/1.1 intra"),
        (OTHER, 40002, SERVER, 80, b"net\r\n"),
        (OTHER, 40003, SERVER, 80, b"POST /admin HTTP/1.1\r\n"),
        (SERVER, 80, OTHER, 40003, b"in"),
        (OTHER, 40004, SERVER, 80, b"...Host: exa"),
        (OTHER, 40004, SERVER, 80, b""),
        (OTHER, 40004, SERVER, 80, b"mple"),
    ]
    frames = [HM.make_frame("tcp", p, s, d, sp, dp) for s, sp, d, dp, p in seg]
    return [(len(f), f) for f in frames]


@pytest.mark.gpu
def test_flow_alerts_with_and_without_seams(tmp_path):
    frames = _capture()
    pcap, strings, rules_file = tmp_path / "split.pcap", tmp_path / "strings.txt", tmp_path / "rules.txt"
    HM.write_pcap(pcap, frames)
    pats = [b"/admin", b"intranet", b"Host:", b"example"]
    strings.write_bytes(b"\n".join(pats) + b"\n")
    rules = [([0], [1]), ([2, 3], []), ([], [0])]
    rules_file.write_text("".join(" ".join([str(i) for i in pos] + ["!" + str(i) for i in neg]) + "\n" for pos, neg in rules))
    pay, meta = HM.capture(frames, "tcp")
    assert len(pay) == len(frames)
    lens = [len(t) for t in pay]
    fo = FM.flow_of(meta)
    n_flows = int(fo.max()) + 1
    hits = MM.hits(MM.starts(pay, pats), len(pats))
    plain = FM.flow_rules(hits, fo, rules, n_flows)
    want = {}
    for reach in (98, 5, 4, 3):
        recs = SM.records(meta, lens, reach)
        seam_hits = MM.hits(MM.starts(SM.payloads(pay, recs), pats), len(pats))
        want[reach] = SM.flow_rules(hits, seam_hits, fo, fo[recs["next"].astype(np.int64)], rules, n_flows)
    # the split /admin fires with the seams, the split intranet bars, and the second "example" is split across three payloads: found by no
    # seam.  /admin leaves 4 bytes in front of its boundary, intranet 5: a reach of 4 still finds the one, a reach of 3 neither
    assert plain.astype(int).tolist() == [[0, 0, 1, 1, 0], [1, 0, 0, 0, 0], [1, 1, 0, 0, 1]]
    assert want[98].astype(int).tolist() == [[1, 0, 0, 1, 0], [1, 0, 0, 0, 0], [0, 1, 0, 0, 1]]
    assert np.array_equal(want[5], want[98]) and want[4].astype(int).tolist() == [[1, 0, 1, 1, 0], [1, 0, 0, 0, 0], [0, 1, 0, 0, 1]]
    assert np.array_equal(want[3], plain)

    def alerts(prog, extra, seams):
        out = tmp_path / f"flow_alerts_{prog}_{seams}.csv"
        env = {k: v for k, v in os.environ.items() if not k.startswith("KMPGPU_")}
        env.update({"KMPGPU_FLOW_ALERTS_FILE": str(out), "KMPGPU_RULES_FILE": str(rules_file)})
        if seams:
            env["KMPGPU_FLOW_SEAMS"] = str(seams)
        r = subprocess.run([os.path.join(_lib.BINDIR, prog), str(pcap), str(strings), *extra, "tcp"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr
        return out.read_text(), r.stdout

    for seams, rows in ((0, plain), (98, want[98]), (4, want[4]), (3, want[3])):
        a, b = alerts("serial", [], seams), alerts("openmp_data", ["1"], seams)
        assert a[0] == b[0] == FM.flow_alerts_file(rows), seams
    # stdout is what it is without the variable (the elapsed time aside)
    strip = lambda s: "".join(l for l in s.splitlines(keepends=True) if not l.startswith("Elapsed time = "))
    assert strip(alerts("serial", [], 98)[1]) == strip(alerts("serial", [], 0)[1])
