"""KMPGPU_DNS_FIELD in bin/serial and bin/openmp_data on a real MI355X: the row outputs are decided on the name buffer, in the capture's
payload numbering; stdout is what it is without the variable.  The expectations come from tests/dns_model.py and tests/match_model.py.

Run on a real MI355X:  python -m pytest tests/test_dns_cli.py -m gpu
"""
import os

import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import run_cli, strip_elapsed  # noqa: E402  (torch first)

import decode_model as DM  # noqa: E402
import dns_model as DNS  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402

PATS = [b"youtube.com", b"doubleclick.net", b"www", b"google"]
RULES = [([0], []), ([1], [2]), ([2, 3], [])]


def rows_files(texts):
    hits = MM.hits(MM.starts(texts, PATS))
    rows = MM.rule_rows(hits, RULES)
    n = len(texts)
    return ("".join(f"{k},{i}\n" for k in range(n) for i in range(len(PATS)) if hits[i, k]),
            "".join(f"{k},{q}\n" for k in range(n) for q in range(len(RULES)) if rows[q, k]))


def test_serial_on_very_big_udp(tmp_path):
    strings, rf = str(tmp_path / "patterns.txt"), str(tmp_path / "rules.txt")
    with open(strings, "wb") as f:
        f.write(b" ".join(PATS) + b"\n")
    with open(rf, "w") as f:
        f.write("0\n1 !2\n2 3\n")
    host = K.HostArena.from_pcap(os.path.join(DATA, "very_big_udp.pcap"), "udp")
    payloads = [bytes(host.payload(k)) for k in range(host.n_pkts)]
    names = [DNS.qname(p) or b"" for p in payloads]
    plain = run_cli("serial", pcap="very_big_udp.pcap", strings=strings)
    assert plain.returncode == 0, plain.stderr
    packets, alerts = tmp_path / "packets.csv", tmp_path / "alerts.csv"
    r = run_cli("serial", pcap="very_big_udp.pcap", strings=strings,
                env_extra={"KMPGPU_DNS_FIELD": "qname", "KMPGPU_RULES_FILE": rf, "KMPGPU_PACKETS_FILE": str(packets), "KMPGPU_ALERTS_FILE": str(alerts)})
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == strip_elapsed(plain.stdout)               # byte for byte what it is without the variable
    want_packets, want_alerts = rows_files(names)
    assert packets.read_text() == want_packets and alerts.read_text() == want_alerts
    assert sum(line.endswith(",0\n") for line in want_alerts.splitlines(keepends=True)) == 4324


@pytest.mark.parametrize("prog, extra", [("serial", ()), ("openmp_data", ("1",))])
def test_command_lines_with_the_prefix(tmp_path, prog, extra):
    """qname,tcp on messages with the 2-byte length in front, next to qname on the same capture, and a payload that is no message"""
    msgs = [DNS.message([b"www", b"youtube", b"com"], tcp_prefix=True), b"youtube.com in the clear", DNS.message([b"ad", b"doubleclick", b"net"], tcp_prefix=True),
            DNS.message([b"www", b"google", b"com"], flags=0x8180, an=1, tail=b"\xc0\x0c", tcp_prefix=True), DNS.message([], tcp_prefix=True)]
    pcap, strings, rf = (str(tmp_path / name) for name in ("dns.pcap", "patterns.txt", "rules.txt"))
    K.write_udp_pcap(pcap, *DM.packed_image(msgs))
    with open(strings, "wb") as f:
        f.write(b" ".join(PATS) + b"\n")
    with open(rf, "w") as f:
        f.write("0\n1 !2\n2 3\n")
    raw_report = K.format_report(PATS, MM.counts(MM.starts(msgs, PATS)))
    for value, tcp in (("qname,tcp", True), ("qname", False)):
        packets, alerts = tmp_path / f"packets_{tcp}.csv", tmp_path / f"alerts_{tcp}.csv"
        r = run_cli(prog, pcap=pcap, strings=strings, extra=extra,
                    env_extra={"KMPGPU_DNS_FIELD": value, "KMPGPU_RULES_FILE": rf, "KMPGPU_PACKETS_FILE": str(packets), "KMPGPU_ALERTS_FILE": str(alerts)})
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == raw_report
        want_packets, want_alerts = rows_files([DNS.qname(p, tcp) or b"" for p in msgs])
        assert packets.read_text() == want_packets and alerts.read_text() == want_alerts
        if tcp:
            assert want_alerts == "0,0\n2,1\n3,2\n"
