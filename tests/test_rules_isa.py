"""What the compiler made of the rules kernel of kmpgpu_scan_rules (no GPU needed: hipcc cross-compiles gfx950).

kmp_rules.hip reads the hit matrix and the rules' term lists with 16-byte loads, several rows in flight per lane, without
scratch or run-time register indexing, at an occupancy that hides the latency of its dependent loads."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def rules_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_rules.hip", str(tmp_path_factory.mktemp("isa")))


def test_rules_kernel_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_rules.hip" in hipsrc.split()


def test_rules_kernel(rules_isa):
    ks = {n: k for n, k in rules_isa.items() if "kmp_rules_kernel" in n}
    assert len(ks) == 1, list(rules_isa)
    k = next(iter(ks.values()))
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    loads = re.findall(r"^\s*(?:global|buffer)_load_(\w+)", k["body"], re.M)
    # the rules' heads and term quads and the matrix rows are all read in 16-byte loads, several rows in flight per lane
    assert loads and set(loads) == {"dwordx4"}, loads
    assert len(loads) >= 4
    assert k["occupancy"] >= 4, k["vgprs"]
