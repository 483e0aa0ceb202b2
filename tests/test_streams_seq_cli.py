"""KMPGPU_FLOW_STREAMS_ORDER in bin/serial and bin/openmp_data (csrc/host/kmp_cli.c) on the GPU: a small TCP capture written here, with a
request whose segments were captured out of order and one retransmitted, whose flow alerts and stream records are what
tests/stream_seq_model.py says under `seq` and, byte for byte, what they are without the variable under `capture`.  (The refusals of the
options stage: tests/test_cli_streams_seq_host.py.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import flow_model as FM
import header_model as HM
import match_model as MM
import stream_model as TM
import stream_seq_model as QM
from multithreading_string_matching_amd import _lib

pytestmark = pytest.mark.gpu

CLIENT, SERVER, OTHER = 0x0A000001, 0xC0A80101, 0x0A000002
PROGS = [("serial", []), ("openmp_data", ["1"])]


def _frame(s, sp, d, dp, payload, seq):
    f = bytearray(HM.make_frame("tcp", payload, s, d, sp, dp))
    f[14 + 20 + 4:14 + 20 + 8] = struct.pack(">I", seq & 0xFFFFFFFF)
    return bytes(f)


def _capture():
    """the client's request in three segments, the last captured first and the middle one twice, sequence numbers across 2^32; the
    server's answers in order; another connection with a hole"""
    isn = 0xFFFFFFFC
    seg = [
        (CLIENT, 40000, SERVER, 80, b"n HTTP/1.1\r\nHost: example\r\n", isn + 9),
        (SERVER, 80, CLIENT, 40000, b"HTTP/1.1 100 Continue\r\n", 500),
        (CLIENT, 40000, SERVER, 80, b"GET /ad", isn),
        (CLIENT, 40000, SERVER, 80, b"mi", isn + 7),
        (SERVER, 80, CLIENT, 40000, b"", 523),
        (CLIENT, 40000, SERVER, 80, b"mi", isn + 7),
        (OTHER, 40002, SERVER, 80, b"POST /adm", 7000),
        (OTHER, 40002, SERVER, 80, b"in HTTP/1.1\r\n", 7012),
    ]
    frames = [_frame(*row) for row in seg]
    return [(len(f), f) for f in frames], np.array([row[5] & 0xFFFFFFFF for row in seg], dtype=np.uint32)


def test_flow_alerts_and_streams_file(tmp_path):
    frames, seq = _capture()
    pcap, strings, rules_file = tmp_path / "reordered.pcap", tmp_path / "strings.txt", tmp_path / "rules.txt"
    HM.write_pcap(pcap, frames)
    pats = [b"/admin", b"Host: example"]
    strings.write_bytes(b"\n".join(pats) + b"\n")
    rules = [([0], []), ([0, 1], []), ([], [0])]
    rules_file.write_text("".join(" ".join([str(i) for i in pos] + ["!" + str(i) for i in neg]) + "\n" for pos, neg in rules))
    pay, meta = HM.capture(frames, "tcp")
    assert len(pay) == len(frames)
    fo = FM.flow_of(meta)
    n_flows = int(fo.max()) + 1
    depth = 1 << 20
    streams, recs, pos, segs, orders, _ = QM.build(pay, meta, seq, depth)
    assert streams[0] == b"GET /admin HTTP/1.1\r\nHost: example\r\n" and orders["dup_bytes"].tolist() == [2, 0, 0]
    assert streams[2] == b"POST /admin HTTP/1.1\r\n" and orders["n_gaps"].tolist() == [0, 0, 1] and orders["gap_bytes"].tolist() == [0, 0, 3]
    want_seq = FM.flow_rules(MM.hits(MM.starts(streams, pats), len(pats)), recs["flow"].astype(np.int64), rules, n_flows)
    crecs, _ = TM.records(meta, [len(t) for t in pay], depth)
    want_cap = FM.flow_rules(MM.hits(MM.starts(TM.payloads(pay, meta, depth), pats), len(pats)), crecs["flow"].astype(np.int64), rules, n_flows)
    # in capture order the client's /admin is not contiguous; in sequence order it is.  The other connection's hole is closed either way
    assert want_cap.astype(int).tolist() == [[0, 1], [0, 0], [1, 0]] and want_seq.astype(int).tolist() == [[1, 1], [1, 0], [0, 0]]

    def line(s, r, o=None):
        head = f"{s},{r['flow']},{r['dir']},{r['first_packet']},{r['last_packet']},{r['n_packets']},{r['bytes']},{r['len']}"
        return head + (f",{o['tcp']},{o['n_gaps']},{o['gap_bytes']},{o['dup_bytes']}" if o is not None else "") + "\n"

    lines_seq = "".join(line(s, r, o) for s, (r, o) in enumerate(zip(recs, orders)))
    lines_cap = "".join(line(s, r) for s, r in enumerate(crecs))
    assert lines_seq.splitlines()[0] == "0,0,0,0,5,4,36,36,1,0,0,2" and lines_cap.splitlines()[0] == "0,0,0,0,5,4,38,38"

    def run(prog, extra, order):
        out, st = tmp_path / f"flow_alerts_{prog}_{order}.csv", tmp_path / f"streams_{prog}_{order}.csv"
        env = {k: v for k, v in os.environ.items() if not k.startswith("KMPGPU_")}
        env.update({"KMPGPU_FLOW_ALERTS_FILE": str(out), "KMPGPU_RULES_FILE": str(rules_file), "KMPGPU_FLOW_STREAMS": "1m",
                    "KMPGPU_STREAMS_FILE": str(st)})
        if order:
            env["KMPGPU_FLOW_STREAMS_ORDER"] = order
        r = subprocess.run([os.path.join(_lib.BINDIR, prog), str(pcap), str(strings), *extra, "tcp"], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stderr
        return out.read_text(), st.read_text(), r.stdout

    strip = lambda s: "".join(l for l in s.splitlines(keepends=True) if not l.startswith("Elapsed time = "))
    for prog, extra in PROGS:
        base = run(prog, extra, None)
        assert base[0] == FM.flow_alerts_file(want_cap) and base[1] == lines_cap
        capture = run(prog, extra, "capture")
        assert capture[:2] == base[:2] and strip(capture[2]) == strip(base[2])       # byte for byte what it is without the variable
        alerts, streams_file, stdout = run(prog, extra, "seq")
        assert alerts == FM.flow_alerts_file(want_seq), prog
        assert streams_file == lines_seq, prog
        assert strip(stdout) == strip(base[2])                  # stdout is what it is without the variables
