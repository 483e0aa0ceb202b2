"""KMPGPU_HTTP_FIELD in bin/serial and bin/openmp_data on a real MI355X: the row outputs are decided on the field buffer (uri: the raw
URI percent-decoded), in the capture's payload numbering; stdout and the flows file are what they are without the variable.  The
expectations come from tests/http_model.py, tests/decode_model.py and tests/match_model.py.

Run on a real MI355X:  python -m pytest tests/test_fields_cli.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import run_cli, strip_elapsed  # noqa: E402  (torch first)

import decode_model as DM  # noqa: E402
import flow_model as FM  # noqa: E402
import http_model as HM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402

PAYLOADS = [b"GET /%61dmin HTTP/1.1\r\nHost: intranet\r\nUser-Agent: curl\r\n\r\n",
            b"GET /index.html HTTP/1.1\r\nReferer: http://intranet/admin\r\n\r\n",
            b"POST /login HTTP/1.1\r\nHost: intranet\r\n\r\nnext=/admin&password=x",
            b"HTTP/1.1 200 OK\r\nServer: intranet\r\n\r\n<a href=/admin>",
            b"GET /admin/users?q=curl HTTP/1.1\r\n\r\n",
            b"not http at all: /admin intranet curl",
            b"GET /a HTTP/1.1\r\nHost: intra"]
PATS = [b"/admin", b"intranet", b"curl"]
RULES = [([0], []), ([1], [2]), ([2], []), ([1], [0])]


def texts_of(value):
    if value is None:
        return PAYLOADS
    if value == "uri":
        return [DM.decode(HM.field(t, "raw_uri") or b"") for t in PAYLOADS]
    return [HM.field(t, value) or b"" for t in PAYLOADS]


@pytest.mark.parametrize("prog, extra", [("serial", ()), ("openmp_data", ("1",))])
def test_command_lines(tmp_path, prog, extra):
    pcap, strings, rf = (str(tmp_path / name) for name in ("http.pcap", "patterns.txt", "rules.txt"))
    K.write_udp_pcap(pcap, *DM.packed_image(PAYLOADS))
    with open(strings, "wb") as f:
        f.write(b" ".join(PATS) + b"\n")
    with open(rf, "w") as f:
        f.write("0\n1 !2\n2\n1 !0\n")
    meta = K.HostArena.from_pcap(pcap, "udp", with_meta=True).meta
    fo = FM.flow_of_np(meta)
    raw_report = K.format_report(PATS, MM.counts(MM.starts(PAYLOADS, PATS)))
    seen = {}
    for value in (None, "uri", "headers", "raw_uri", "body"):
        texts = texts_of(value)
        hits = MM.hits(MM.starts(texts, PATS))
        rows = MM.rule_rows(hits, RULES)
        out = {name: tmp_path / f"{name}_{value}.csv" for name in ("packets", "alerts", "flow_alerts", "flows")}
        env = {"KMPGPU_RULES_FILE": rf, "KMPGPU_PACKETS_FILE": str(out["packets"]), "KMPGPU_ALERTS_FILE": str(out["alerts"]),
               "KMPGPU_FLOW_ALERTS_FILE": str(out["flow_alerts"]), "KMPGPU_FLOWS_FILE": str(out["flows"])}
        if value:
            env["KMPGPU_HTTP_FIELD"] = value
        r = run_cli(prog, pcap=pcap, strings=strings, extra=extra, env_extra=env)
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == raw_report                                # byte for byte what it is without the variable
        assert out["packets"].read_text() == "".join(f"{k},{i}\n" for k in range(len(PAYLOADS)) for i in range(len(PATS)) if hits[i, k])
        assert out["alerts"].read_text() == "".join(f"{k},{q}\n" for k in range(len(PAYLOADS)) for q in range(len(RULES)) if rows[q, k])
        assert out["flow_alerts"].read_text() == FM.flow_alerts_file(FM.flow_rules(hits, fo, RULES))
        seen[value] = {name: path.read_text() for name, path in out.items()}
    assert len({s["flows"] for s in seen.values()}) == 1 and seen[None]["flows"] != ""
    # `/admin` (rule 0): everywhere but in the escaped request line as captured; in the URI of payloads 0 and 4 only; in no header but the Referer:
    assert [int(line.split(",")[0]) for line in seen[None]["alerts"].splitlines() if line.endswith(",0")] == [1, 2, 3, 4, 5]
    assert [int(line.split(",")[0]) for line in seen["uri"]["alerts"].splitlines() if line.endswith(",0")] == [0, 4]
    assert [int(line.split(",")[0]) for line in seen["raw_uri"]["alerts"].splitlines() if line.endswith(",0")] == [4]
    assert [int(line.split(",")[0]) for line in seen["headers"]["alerts"].splitlines() if line.endswith(",0")] == [1]
    assert [int(line.split(",")[0]) for line in seen["body"]["alerts"].splitlines() if line.endswith(",0")] == [2, 3]
