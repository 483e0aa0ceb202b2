"""What the compiler made of the byte-test kernels of kmpgpu_scan_bytetests (no GPU needed: hipcc cross-compiles gfx950).

kmp_bytetests.hip: the absolute kernel -- a lane per payload, the tests out of LDS, the field from one or two aligned dwords, the rows
written in 16-byte pieces -- in its two instantiations (strlen rule, whole payloads), and the relative kernel, a sweep as the relation
kernel's.  No scratch, no run-time register indexing, and registers for at least the occupancy the rules kernel is held to."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_bytetests.hip", str(tmp_path_factory.mktemp("isa")))


def test_bytetests_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_bytetests.hip" in hipsrc.split()


def test_the_file_holds_three_kernels(isa):
    assert len(isa) == 3, list(isa)
    assert sum("kmp_bytetests_abs_kernel" in n for n in isa) == 2 and sum("kmp_bytetests_rel_kernel" in n for n in isa) == 1


def test_absolute_kernels(isa):
    ks = {n: k for n, k in isa.items() if "kmp_bytetests_abs_kernel" in n}
    assert len(ks) == 2, list(isa)
    nul_loads = {}
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        # a row leaves in 16-byte pieces, and nothing else is stored
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        # the field comes in aligned dwords, never byte by byte
        assert "dword" in loads and not {"ubyte", "sbyte", "ushort", "sshort"} & set(loads), (name, loads)
        assert k["occupancy"] >= 4, (name, k["vgprs"])     # (what tests/test_rules_isa.py asks of the rules kernel)
        nul_loads[name] = loads.count("dwordx4")
    # the search for the first 0x00 (16-byte loads of the text) is compiled out of the whole-payload instantiation: what is left of
    # dwordx4 loads there is the staging of the tests' records
    whole = next(n for n in ks if "ILb1E" in n)
    strlen = next(n for n in ks if "ILb0E" in n)
    assert nul_loads[strlen] > nul_loads[whole], nul_loads


def test_relative_kernel(isa):
    ks = {n: k for n, k in isa.items() if "kmp_bytetests_rel_kernel" in n}
    assert len(ks) == 1, list(isa)
    k = next(iter(ks.values()))
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    # one row word per (test, column word), from lane 0
    stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
    assert stores == ["dwordx2"], stores
    assert k["occupancy"] >= 4, k["vgprs"]
