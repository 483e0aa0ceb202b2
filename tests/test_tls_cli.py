"""KMPGPU_TLS_FIELD in bin/serial and bin/openmp_data on a real MI355X: the row outputs are decided on the server-name or the ALPN buffer,
in the capture's payload numbering; stdout is what it is without the variable.  The expectations come from tests/tls_model.py and
tests/match_model.py, and the Python route (GpuMatcher.load_tls, then the same patterns and rules) must give the same rows.

Run on a real MI355X:  python -m pytest tests/test_tls_cli.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import run_cli, strip_elapsed  # noqa: E402  (torch first)

import decode_model as DM  # noqa: E402
import match_model as MM  # noqa: E402
import tls_model as TLS  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

PATS = [b"example.com", b"h2", b"www", b"http/1.1", b"h2,http/1.1"]
RULES = [([0], []), ([1], [3]), ([2, 0], []), ([4], [])]
H, SNI, ALPN, EXT = TLS.hello, TLS.sni_ext, TLS.alpn_ext, TLS.ext


def capture():
    return [H([SNI(b"www.example.com"), ALPN([b"h2", b"http/1.1"])]), b"example.com and h2 in the clear", H([ALPN([b"h2"]), SNI(b"example.com")], sid=0),
            H([EXT(100, b"www.example.com h2")]), H([SNI(b"www.example.org"), ALPN([b"http/1.1"])]), H([SNI(b"example.com"), ALPN([b"h2", b"http/1.1"])])[:-3],
            b"", H([SNI(b"EXAMPLE.COM"), ALPN([b"h2", b"http/1.1", b"h3"])], sid=7)]


def rows_files(texts):
    hits = MM.hits(MM.starts(texts, PATS))
    rows = MM.rule_rows(hits, RULES)
    n = len(texts)
    return hits, rows, ("".join(f"{k},{i}\n" for k in range(n) for i in range(len(PATS)) if hits[i, k]),
                        "".join(f"{k},{q}\n" for k in range(n) for q in range(len(RULES)) if rows[q, k]))


@pytest.mark.parametrize("prog, extra", [("serial", ()), ("openmp_data", ("1",))])
def test_command_lines(tmp_path, prog, extra):
    msgs = capture()
    pcap, strings, rf = (str(tmp_path / name) for name in ("tls.pcap", "patterns.txt", "rules.txt"))
    K.write_udp_pcap(pcap, *DM.packed_image(msgs))
    with open(strings, "wb") as f:
        f.write(b" ".join(PATS) + b"\n")
    with open(rf, "w") as f:
        f.write("0\n1 !3\n2 0\n4\n")
    raw_report = K.format_report(PATS, MM.counts(MM.starts(msgs, PATS)))
    with GpuMatcher(0) as src, GpuMatcher(0) as dst:
        src.load_arena(K.HostArena.from_payloads(msgs))
        dst.set_patterns(PATS)
        dst.set_rules(RULES)
        for value in ("sni", "alpn"):
            packets, alerts = tmp_path / f"packets_{value}.csv", tmp_path / f"alerts_{value}.csv"
            r = run_cli(prog, pcap=pcap, strings=strings, extra=extra,
                        env_extra={"KMPGPU_TLS_FIELD": value, "KMPGPU_RULES_FILE": rf, "KMPGPU_PACKETS_FILE": str(packets), "KMPGPU_ALERTS_FILE": str(alerts)})
            assert r.returncode == 0, r.stderr
            assert strip_elapsed(r.stdout) == raw_report                         # the report stays the capture's
            hits, rows, (want_packets, want_alerts) = rows_files([TLS.field_of(p, value) or b"" for p in msgs])
            assert packets.read_text() == want_packets and alerts.read_text() == want_alerts
            if value == "sni":
                assert want_alerts == "0,0\n0,2\n2,0\n5,0\n"
            else:
                assert want_alerts == "0,3\n2,1\n7,3\n"
            # the Python route
            dst.load_tls(src, value)
            assert np.array_equal(dst.scan_packets(hits=True)["hits"], hits) and np.array_equal(dst.scan_rules(hits=True)["hits"], rows)
