"""KMPGPU_FLOWS_FILE / KMPGPU_FLOW_ALERTS_FILE in the options stage of bin/serial and bin/openmp_data (csrc/host/kmp_cli.c: load_options) on
a machine without a GPU: every refusal is made before any GPU work, with exit code 1, nothing on stdout and the message on stderr to the
byte.  bin/openmp_task ignores the variables."""
import os

import pytest

from conftest import DATA

from test_cli_options_host import ENOENT, TOGETHER, refused, run

ONE_SHARD = "KMPGPU_FLOWS_FILE and KMPGPU_FLOW_ALERTS_FILE need one shard, thread_number is {}: a flow would be cut at a shard's edge\n"
NEEDS_RULES = "KMPGPU_FLOW_ALERTS_FILE goes together with KMPGPU_RULES_FILE: it is not set\n"
PROGS = [("serial", []), ("openmp_data", ["1"])]


@pytest.fixture
def files(tmp_path):
    rules = tmp_path / "rules.txt"
    rules.write_text("0 !1\n2\n")
    return {"rules": rules, "flows": tmp_path / "flows.csv", "flow_alerts": tmp_path / "flow_alerts.csv", "alerts": tmp_path / "alerts.csv",
            "unwritable": tmp_path / "no_such_dir" / "out.csv", "missing": tmp_path / "no_such_file.txt"}


def test_more_than_one_shard(files):
    f = files
    for shards in ("2", "8"):
        refused("openmp_data", [shards], {"FLOWS_FILE": f["flows"]}, ONE_SHARD.format(shards))
        refused("openmp_data", [shards], {"FLOW_ALERTS_FILE": f["flow_alerts"], "RULES_FILE": f["rules"]}, ONE_SHARD.format(shards))
        # the shards come first: before the missing rules file and before the paths are probed
        refused("openmp_data", [shards], {"FLOW_ALERTS_FILE": f["unwritable"]}, ONE_SHARD.format(shards))
    assert not f["flows"].exists() and not f["flow_alerts"].exists()


@pytest.mark.parametrize("prog,extra", PROGS)
def test_flow_alerts_need_rules_and_paths_must_be_writable(files, prog, extra):
    f = files
    refused(prog, extra, {"FLOW_ALERTS_FILE": f["flow_alerts"]}, NEEDS_RULES)
    refused(prog, extra, {"FLOW_ALERTS_FILE": f["flow_alerts"], "FLOWS_FILE": f["flows"], "FLOWS_DIRECTED": "1"}, NEEDS_RULES)
    assert not f["flows"].exists() and not f["flow_alerts"].exists()
    # an alerts file without rules is refused as ever; rules with the flow alerts alone are enough
    refused(prog, extra, {"FLOW_ALERTS_FILE": f["flow_alerts"], "ALERTS_FILE": f["alerts"]}, TOGETHER.format("KMPGPU_RULES_FILE"))
    refused(prog, extra, {"FLOW_ALERTS_FILE": f["flow_alerts"], "RULES_FILE": f["missing"]}, f"error reading rules file {f['missing']}: {f['missing']}: {ENOENT}\n")
    refused(prog, extra, {"FLOWS_FILE": f["unwritable"]}, f"KMPGPU_FLOWS_FILE: {ENOENT}\n")
    refused(prog, extra, {"FLOWS_FILE": f["flows"], "FLOW_ALERTS_FILE": f["unwritable"], "RULES_FILE": f["rules"]}, f"KMPGPU_FLOW_ALERTS_FILE: {ENOENT}\n")
    # an empty value is no value
    refused(prog, extra, {"FLOW_ALERTS_FILE": "", "RULES_FILE": f["rules"]}, TOGETHER.format("KMPGPU_ALERTS_FILE"))


@pytest.mark.parametrize("prog,extra", PROGS)
def test_good_variables_pass_the_options_stage(files, prog, extra):
    """... and end where a plain run ends: without a device with exit code 2 and the device message, the two files started empty"""
    import torch
    f = files
    r = run(prog, extra, {"FLOWS_FILE": f["flows"], "FLOW_ALERTS_FILE": f["flow_alerts"], "RULES_FILE": f["rules"]})
    assert f["flows"].exists() and f["flow_alerts"].exists()
    if torch.cuda.is_available():
        assert r.returncode == 0 and f["flows"].stat().st_size > 0, r.stderr
    else:
        assert (r.returncode, r.stdout) == (2, "") and r.stderr.startswith("no MI355X device: "), r.stderr
        assert f["flows"].stat().st_size == 0 and f["flow_alerts"].stat().st_size == 0


def test_openmp_task_ignores_the_variables(files):
    import torch
    f = files
    r = run("openmp_task", [], {"FLOWS_FILE": f["unwritable"], "FLOW_ALERTS_FILE": f["flow_alerts"]})
    assert not f["flow_alerts"].exists() and "KMPGPU_FLOW" not in r.stderr
    assert r.returncode == (0 if torch.cuda.is_available() else 2), r.stderr
