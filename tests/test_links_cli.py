"""KMPGPU_LINKS_FILE in bin/serial and bin/openmp_data on a real MI355X: rules over links of two buffers on a small HTTP capture the test
writes itself; the alerts file must equal, byte for byte, what the Python route (GpuMatcher.set_links / link_rows / scan_rules) gives for
the same payloads, and both are what tests/http_model.py and tests/decode_model.py say.

Run on a real MI355X:  python -m pytest tests/test_links_cli.py -m gpu
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import run_cli, strip_elapsed  # noqa: E402  (torch first)

import decode_model as DM  # noqa: E402
import http_model as HM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402

PATS = [b"/admin", b"evil", b"intranet", b"POST"]
LINKS = "# the decoded URI and the body\nhttp:uri 0\nhttp:body 1\n"
RULES = "l0 l1 3\nl1 !l0\n2 !l1\n"


def capture():
    pay = []
    for k in range(90):
        uri = [b"/admin/x", b"/%61dmin", b"/index", b"/adm%69n?evil"][k % 4]
        body = [b"an evil body", b"plain /admin", b""][k % 3]
        verb = [b"POST", b"GET"][k % 5 == 0]
        pay.append(verb + b" " + uri + b" HTTP/1.1\r\nHost: " + [b"intranet", b"example.org"][k % 2] + b"\r\n\r\n" + body)
    return pay + [b"evil /admin POST but no request", b"\x00POST"]


def python_route(pay):
    ms = [GpuMatcher(0) for _ in range(4)]
    cap, raw, uri, body = ms
    try:
        for m in ms:
            m.set_patterns(PATS)
        cap.load_arena(K.HostArena.from_payloads(pay))
        raw.load_fields(cap, "raw_uri")
        uri.load_decoded(raw)
        body.load_fields(cap, "body")
        uri.set_rules([([0], [])])
        body.set_rules([([1], [])])
        cap.set_links(2)
        cap.link_rows(0, uri, "rules")
        cap.link_rows(1, body, "rules")
        cap.set_rules([([cap.link(0), cap.link(1), 3], []), ([cap.link(1)], [cap.link(0)]), ([2], [cap.link(1)])])
        return cap.scan_rules(hits=True)["hits"]
    finally:
        for m in ms:
            m.close()


def alerts_text(rows):
    return "".join(f"{k},{q}\n" for k in range(rows.shape[1]) for q in range(rows.shape[0]) if rows[q, k])


@pytest.mark.parametrize("prog, extra", [("serial", ()), ("openmp_data", ("2",))])
def test_alerts_equal_the_python_route(tmp_path, prog, extra):
    pay = capture()
    pcap, strings, rf, lf = (str(tmp_path / name) for name in ("http.pcap", "patterns.txt", "rules.txt", "links.txt"))
    K.write_udp_pcap(pcap, *DM.packed_image(pay))
    for path, text in ((strings, b" ".join(PATS) + b"\n"), (rf, RULES.encode()), (lf, LINKS.encode())):
        with open(path, "wb") as f:
            f.write(text)
    alerts = tmp_path / "alerts.csv"
    r = run_cli(prog, pcap=pcap, strings=strings, extra=extra, env_extra={"KMPGPU_LINKS_FILE": lf, "KMPGPU_RULES_FILE": rf, "KMPGPU_ALERTS_FILE": str(alerts)})
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == K.format_report(PATS, MM.counts(MM.starts(pay, PATS)))         # stdout is the capture's own
    rows = python_route(pay)
    assert alerts.read_text() == alerts_text(rows)
    # ... and both are what the models of the fields and of the decoding say
    own = MM.hits(MM.starts(pay, PATS))
    l0 = np.array([b"/admin" in DM.decode(HM.field(p, "raw_uri") or b"").split(b"\0")[0] for p in pay])
    l1 = np.array([b"evil" in (HM.field(p, "body") or b"").split(b"\0")[0] for p in pay])
    want = np.stack([l0 & l1 & own[3], l1 & ~l0, own[2] & ~l1])
    assert np.array_equal(rows, want) and want.sum(axis=1).min() > 0
