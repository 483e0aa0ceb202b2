"""KMPGPU_THRESHOLDS_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options) on a machine without
a GPU: every refusal it makes before any GPU work, with exit code 1, nothing on stdout and the message on stderr to the byte; and one
consistent setting, which passes the whole stage and only then looks for a device.  bin/openmp_task ignores the variable."""
import os
import subprocess

import pytest

from conftest import DATA

from multithreading_string_matching_amd import _lib

PROGS = [("serial", []), ("openmp_data", ["1"])]
NEEDS = "KMPGPU_THRESHOLDS_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: {} is not set\n"
SHARDS = "KMPGPU_THRESHOLDS_FILE needs one shard, thread_number is 2: a tracker's window would be cut at a shard's edge\n"
DEVICE_EXTRACT = "KMPGPU_THRESHOLDS_FILE does not go together with KMPGPU_DEVICE_EXTRACT=1: the device extractor keeps no timestamps\n"
NOT_WITH = {
    "FLOWBITS_FILE": "thresholds over flow-bit alerts are not defined",
    "FLOW_ALERTS_FILE": "the rules per flow know no thresholds",
    "FLOW_SEAMS": "seams have no time",
    "FLOW_STREAMS": "streams have no time",
    "DECODE": "decoded payloads keep no timestamps in this program",
    "EXPORT_FILE": "the export selects by the rules without their thresholds",
}
BAD_FILES = [
    ("0 by_src at_least 5 60\nx by_src at_least 5 60\n", "line 2: 'x' is not a rule index"),
    ("2 by_src at_least 5 60\n", "line 1: rule 2 of 2"),
    ("# only a rule\n1\n", "line 2: rule 1 has no track (by_rule, by_src, by_dst, by_flow)"),
    ("0 by_pair at_least 5 60\n", "line 1: 'by_pair' is none of by_rule by_src by_dst by_flow"),
    ("0 by_src\n", "line 1: rule 0 has no type (at_least, at_most, exactly)"),
    ("0 by_src\n\n1 by_dst limit 5 60\n", "line 1: rule 0 has no type (at_least, at_most, exactly)"),
    ("0 by_src at_least 5 60\n\n1 by_dst limit 5 60\n", "line 3: 'limit' is none of at_least at_most exactly"),
    ("0 by_src at_least\n", "line 1: rule 0 has no count"),
    ("0 by_src at_least 0 60\n", "line 1: '0' is not a count in 1..4294967295"),
    ("0 by_src at_least 4294967296 60\n", "line 1: '4294967296' is not a count in 1..4294967295"),
    ("0 by_src at_least 5\n", "line 1: rule 0 has no window (seconds, or all)"),
    ("0 by_src at_least 5 1m\n", "line 1: '1m' is neither all nor seconds with at most 6 fraction digits"),
    ("0 by_src at_least 5 0.1234567\n", "line 1: '0.1234567' is neither all nor seconds with at most 6 fraction digits"),
    ("0 by_src at_least 5 18446744073709.551615\n", "line 1: '18446744073709.551615' seconds are more than 2^64 - 2 microseconds"),
    ("0 by_src at_least 5 0.0\n", "line 1: '0.0': a window of 0 holds no payload"),
    ("0 by_src at_least 5 60 s\n", "line 1: 's' follows the window"),
]


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
    out = {name: tmp_path / (name + ".txt") for name in ("rules", "thresholds", "flowbits", "alerts", "other")}
    out["rules"].write_text("0 !1\n2\n")
    out["thresholds"].write_text("# the third hit of rule 0 from one address within a second, and rule 1 once per flow\n0 by_src at_least 3 1\n1 by_flow at_most 1 all\n")
    out["flowbits"].write_text("0 set:seen\n")
    return out


def thr_env(f, **more):
    return dict({"RULES_FILE": f["rules"], "ALERTS_FILE": f["alerts"], "THRESHOLDS_FILE": f["thresholds"]}, **more)


@pytest.mark.parametrize("prog,extra", PROGS)
def test_variables_it_needs_and_does_not_go_with(files, prog, extra):
    f = files
    refused(prog, extra, {"THRESHOLDS_FILE": f["thresholds"]}, NEEDS.format("KMPGPU_RULES_FILE"))
    refused(prog, extra, {"THRESHOLDS_FILE": f["thresholds"], "RULES_FILE": f["rules"], "EXPORT_FILE": f["other"]}, NEEDS.format("KMPGPU_ALERTS_FILE"))
    refused(prog, extra, {"THRESHOLDS_FILE": f["thresholds"], "RULES_FILE": f["rules"], "FLOW_ALERTS_FILE": f["other"]}, NEEDS.format("KMPGPU_ALERTS_FILE"))
    values = {"FLOWBITS_FILE": f["flowbits"], "FLOW_ALERTS_FILE": f["other"], "FLOW_SEAMS": 8, "FLOW_STREAMS": 4096, "DECODE": "percent",
              "EXPORT_FILE": f["other"]}
    for var, why in NOT_WITH.items():
        refused(prog, extra, thr_env(f, **{var: values[var]}), f"KMPGPU_THRESHOLDS_FILE does not go together with KMPGPU_{var}: {why}\n")
    # ... whatever else the other variable would have been refused for
    refused(prog, extra, thr_env(f, FLOW_SEAMS="nonsense"), f"KMPGPU_THRESHOLDS_FILE does not go together with KMPGPU_FLOW_SEAMS: {NOT_WITH['FLOW_SEAMS']}\n")
    refused(prog, extra, thr_env(f, DEVICE_EXTRACT=1), DEVICE_EXTRACT)
    assert not f["alerts"].exists() and not f["other"].exists()


def test_more_than_one_shard_is_refused(files):
    refused("openmp_data", ["2"], thr_env(files), SHARDS)


@pytest.mark.parametrize("prog,extra", PROGS)
@pytest.mark.parametrize("text,message", BAD_FILES)
def test_files_that_do_not_parse(files, prog, extra, text, message):
    files["thresholds"].write_text(text)
    refused(prog, extra, thr_env(files), f"error reading thresholds file {files['thresholds']}: {message}\n")
    assert not files["alerts"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_a_file_that_cannot_be_opened(files, prog, extra):
    missing = files["thresholds"].with_suffix(".missing")
    refused(prog, extra, thr_env(files, THRESHOLDS_FILE=missing), f"error reading thresholds file {missing}: {missing}: No such file or directory\n")


@pytest.mark.parametrize("prog,extra", PROGS)
def test_a_consistent_setting_passes_the_stage(files, prog, extra):
    """... and an empty value is an unset variable, and DEVICE_EXTRACT=0 is no device extractor.  Past load_options the program looks for a
    device: exit code 2 and a message about the GPU where there is none, a normal run where there is one."""
    for env in (thr_env(files), thr_env(files, FLOWS_DIRECTED=1), thr_env(files, DEVICE_EXTRACT=0), {"THRESHOLDS_FILE": ""}):
        r = run(prog, extra, env)
        assert r.returncode in (0, 2) and "KMPGPU_THRESHOLDS_FILE" not in r.stderr and "thresholds" not in r.stderr, r.stderr
        assert (r.returncode == 0) == r.stdout.startswith("Printing the number of appereances")


def test_openmp_task_ignores_the_variable():
    r = run("openmp_task", ["1"], {"THRESHOLDS_FILE": "/no_such_dir/thresholds.txt"})
    assert r.returncode in (0, 2) and "KMPGPU_THRESHOLDS_FILE" not in r.stderr, r.stderr
