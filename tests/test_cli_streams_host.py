"""KMPGPU_FLOW_STREAMS and KMPGPU_STREAMS_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options) on
a machine without a GPU: every refusal it makes before any GPU work, with exit code 1, nothing on stdout and the message on stderr to the
byte; and one consistent setting, which passes the whole stage and only then looks for a device.  bin/openmp_task ignores the variables."""
import os
import subprocess

import pytest

from conftest import DATA

from multithreading_string_matching_amd import _lib

PROGS = [("serial", []), ("openmp_data", ["1"])]
VALUE = 'KMPGPU_FLOW_STREAMS is "{}": a depth of 1..1073741824 bytes is needed\n'
NO_ALERTS = "KMPGPU_FLOW_STREAMS goes together with KMPGPU_FLOW_ALERTS_FILE: it is not set\n"
NOT_WITH = {
    "FLOW_SEAMS": "KMPGPU_FLOW_STREAMS does not go together with KMPGPU_FLOW_SEAMS: streams hold everything seams hold, up to the cut\n",
    "DECODE": "KMPGPU_FLOW_STREAMS does not go together with KMPGPU_DECODE: decoded streams are not wired in this program\n",
}
FILE_ALONE = "KMPGPU_STREAMS_FILE goes together with KMPGPU_FLOW_STREAMS: it is not set\n"
SHARDS = "KMPGPU_FLOWS_FILE and KMPGPU_FLOW_ALERTS_FILE need one shard, thread_number is 2: a flow would be cut at a shard's edge\n"


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
    out = {"rules": tmp_path / "rules.txt"}
    out["rules"].write_text("0 !1\n2\n")
    for name in ("flow_alerts", "streams"):
        out[name] = tmp_path / (name + ".csv")
    return out


def flow_env(f, **more):
    return dict({"RULES_FILE": f["rules"], "FLOW_ALERTS_FILE": f["flow_alerts"]}, **more)


@pytest.mark.parametrize("prog,extra", PROGS)
@pytest.mark.parametrize("value", ["0", "-1", "1073741825", "1025m", "1g", "64K", "64 k", "1.5", "0x10", "all", "18446744073709551617"])
def test_values_that_are_no_depth(files, prog, extra, value):
    refused(prog, extra, flow_env(files, FLOW_STREAMS=value), VALUE.format(value))
    refused(prog, extra, flow_env(files, FLOW_STREAMS=value, STREAMS_FILE=files["streams"]), VALUE.format(value))
    assert not files["streams"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_variables_it_needs_and_does_not_go_with(files, prog, extra):
    f = files
    refused(prog, extra, {"FLOW_STREAMS": 4096}, NO_ALERTS)
    refused(prog, extra, {"FLOW_STREAMS": "nonsense"}, NO_ALERTS)                # the flow alerts file is looked at first
    refused(prog, extra, {"FLOW_STREAMS": 4096, "RULES_FILE": f["rules"], "ALERTS_FILE": f["flow_alerts"], "FLOWS_FILE": f["rules"].with_suffix(".flows")}, NO_ALERTS)
    refused(prog, extra, flow_env(f, FLOW_STREAMS=4096, FLOW_SEAMS=8), NOT_WITH["FLOW_SEAMS"])
    refused(prog, extra, flow_env(f, FLOW_STREAMS=4096, DECODE="percent"), NOT_WITH["DECODE"])
    refused(prog, extra, flow_env(f, FLOW_STREAMS="64k", DECODE="percent+plus", STREAMS_FILE=f["streams"]), NOT_WITH["DECODE"])
    # the streams file: not without the streams, and not on a path that cannot be written
    refused(prog, extra, {"STREAMS_FILE": f["streams"]}, FILE_ALONE)
    refused(prog, extra, flow_env(f, STREAMS_FILE=f["streams"]), FILE_ALONE)
    assert not f["streams"].exists()
    r = run(prog, extra, flow_env(f, FLOW_STREAMS=4096, STREAMS_FILE=f["streams"].parent / "no_such_dir" / "streams.csv"))
    assert (r.returncode, r.stdout) == (1, "") and r.stderr.startswith("KMPGPU_STREAMS_FILE: "), r.stderr


def test_more_than_one_shard_is_refused(files):
    refused("openmp_data", ["2"], flow_env(files, FLOW_STREAMS=4096, STREAMS_FILE=files["streams"]), SHARDS)
    assert not files["streams"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_a_consistent_setting_passes_the_stage(files, prog, extra):
    """... and an empty value is an unset variable.  Past load_options the program looks for a device: exit code 2 and a message
    about the GPU where there is none, a normal run where there is one."""
    f = files
    for env in (flow_env(f, FLOW_STREAMS="1m", STREAMS_FILE=f["streams"]), flow_env(f, FLOW_STREAMS=1073741824),
                {"FLOW_STREAMS": "", "STREAMS_FILE": ""}):
        r = run(prog, extra, env)
        assert r.returncode in (0, 2) and "KMPGPU_FLOW_STREAMS" not in r.stderr and "KMPGPU_STREAMS_FILE" not in r.stderr, r.stderr
        assert (r.returncode == 0) == r.stdout.startswith("Printing the number of appereances")


def test_openmp_task_ignores_the_variables():
    r = run("openmp_task", ["1"], {"FLOW_STREAMS": "nonsense", "STREAMS_FILE": "/no_such_dir/streams.csv"})
    assert r.returncode in (0, 2) and "KMPGPU_FLOW_STREAMS" not in r.stderr and "KMPGPU_STREAMS_FILE" not in r.stderr, r.stderr
