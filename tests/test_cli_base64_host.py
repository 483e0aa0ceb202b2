"""KMPGPU_BASE64 in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options) on a machine without a GPU:
every refusal it makes before any GPU work, with exit code 1, nothing on stdout and the message on stderr to the byte; and one
consistent setting, which passes the whole stage and only then looks for a device.  bin/openmp_task ignores the variable."""
import os
import subprocess

import pytest

from conftest import DATA

from multithreading_string_matching_amd import _lib

PROGS = [("serial", []), ("openmp_data", ["1"])]
VALUE = 'KMPGPU_BASE64 is "{}": <min_run> or <min_run>,url with a min_run of 4..255 is needed\n'
REASON = {
    "DECODE": "one decoding per run; at the library, kmpgpu_load_decoded over the base64 context does both",
    "HTTP_FIELD": "base64 in a field buffer is not wired in this program",
    "OFFSETS_FILE": "offsets in decoded payloads are not mapped back to the capture's",
    "EXPORT_FILE": "the export selects and writes the payloads as captured",
    "FLOW_SEAMS": "decoded seams do not exist",
    "FLOW_STREAMS": "base64 in streams is not wired in this program",
    "FLOWBITS_FILE": "flow bits over base64-decoded payloads are not wired in this program",
    "THRESHOLDS_FILE": "base64-decoded payloads keep no timestamps in this program",
}
NOT_WITH = {k: f"KMPGPU_BASE64 does not go together with KMPGPU_{k}: {v}\n" for k, v in REASON.items()}
NO_EFFECT = "KMPGPU_BASE64 has no effect without KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE\n"


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
    out = {"rules": tmp_path / "rules.txt", "flowbits": tmp_path / "flowbits.txt", "thresholds": tmp_path / "thresholds.txt"}
    out["rules"].write_text("0 !1\n2\n")
    out["flowbits"].write_text("0 set:seen\n1 isset:seen\n")
    out["thresholds"].write_text("0 by_src at_least 2 60\n")
    for name in ("offsets", "packets", "alerts", "flow_alerts"):
        out[name] = tmp_path / (name + ".csv")
    out["export"] = tmp_path / "export.pcap"
    return out


@pytest.mark.parametrize("prog,extra", PROGS)
@pytest.mark.parametrize("value", ["3", "0", "256", "-16", "+16", " 16", "16 ", "16,", "16,URL", "16,url ", "16;url", "url", "percent", "0x10",
                                   "99999999999999999999"])
def test_values_that_are_refused(files, prog, extra, value):
    refused(prog, extra, {"BASE64": value, "PACKETS_FILE": files["packets"]}, VALUE.format(value))
    refused(prog, extra, {"BASE64": value}, VALUE.format(value))                  # the value is looked at first


@pytest.mark.parametrize("prog,extra", PROGS)
@pytest.mark.parametrize("value", ["16", "4,url"])
def test_variables_it_does_not_go_with(files, prog, extra, value):
    f = files
    rows = {"PACKETS_FILE": f["packets"]}
    alerts = {"RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"]}
    refused(prog, extra, {"BASE64": value}, NO_EFFECT)
    refused(prog, extra, {"BASE64": value, "FLOWS_FILE": f["alerts"]}, NO_EFFECT)          # the flows file is no row output
    refused(prog, extra, {"BASE64": value, **rows, "DECODE": "percent"}, NOT_WITH["DECODE"])
    refused(prog, extra, {"BASE64": value, **rows, "HTTP_FIELD": "headers"}, NOT_WITH["HTTP_FIELD"])
    refused(prog, extra, {"BASE64": value, **rows, "OFFSETS_FILE": f["offsets"]}, NOT_WITH["OFFSETS_FILE"])
    refused(prog, extra, {"BASE64": value, "OFFSETS_FILE": f["offsets"]}, NOT_WITH["OFFSETS_FILE"])
    refused(prog, extra, {"BASE64": value, **rows, "EXPORT_FILE": f["export"]}, NOT_WITH["EXPORT_FILE"])
    flow = {"RULES_FILE": f["rules"], "FLOW_ALERTS_FILE": f["flow_alerts"]}
    refused(prog, extra, {"BASE64": value, **flow, "FLOW_SEAMS": 8}, NOT_WITH["FLOW_SEAMS"])
    refused(prog, extra, {"BASE64": value, **flow, "FLOW_STREAMS": 4096}, NOT_WITH["FLOW_STREAMS"])
    refused(prog, extra, {"BASE64": value, **alerts, "FLOWBITS_FILE": f["flowbits"]}, NOT_WITH["FLOWBITS_FILE"])
    refused(prog, extra, {"BASE64": value, **alerts, "THRESHOLDS_FILE": f["thresholds"]}, NOT_WITH["THRESHOLDS_FILE"])
    assert not f["offsets"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_a_consistent_setting_passes_the_stage(files, prog, extra):
    """... and an empty value is an unset variable.  Past load_options the program looks for a device: exit code 2 and a message
    about the GPU where there is none, a normal run where there is one."""
    f = files
    for env in ({"BASE64": "16,url", "PACKETS_FILE": f["packets"], "RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"],
                 "FLOW_ALERTS_FILE": f["flow_alerts"]}, {"BASE64": "255", "PACKETS_FILE": f["packets"]}, {"BASE64": ""}):
        r = run(prog, extra, env)
        assert r.returncode in (0, 2) and "KMPGPU_BASE64" not in r.stderr, r.stderr
        assert (r.returncode == 0) == r.stdout.startswith("Printing the number of appereances")


def test_openmp_task_ignores_the_variable():
    r = run("openmp_task", ["1"], {"BASE64": "nonsense"})
    assert r.returncode in (0, 2) and "KMPGPU_BASE64" not in r.stderr, r.stderr
