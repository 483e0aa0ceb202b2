"""What the compiler made of the grouped regex kernel (no GPU needed: hipcc cross-compiles gfx950).

kmp_regex_groups.hip: the shape of kmp_regex.hip with KMP_RXG_TILE expressions per tile -- two instantiations, no scratch, no run-time
register indexing, 16-byte stores and loads, and registers for the occupancy the row kernels are held to.  kmp_regex.hip keeps its two."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_regex_groups.hip", str(tmp_path_factory.mktemp("isa")))


def test_grouped_kernel_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC")).split()
    assert "kmp_regex_groups.hip" in hipsrc and "kmp_regex.hip" in hipsrc


def test_the_file_holds_two_instantiations(isa, tmp_path):
    assert len(isa) == 2, list(isa)
    assert all("kmp_regex_groups_kernel" in n for n in isa)
    assert sum("ILb1E" in n for n in isa) == 1 and sum("ILb0E" in n for n in isa) == 1
    assert len(_isa("kmp_regex.hip", str(tmp_path))) == 2


def test_grouped_regex_kernels(isa):
    for name, k in isa.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        assert "dwordx4" in loads and not {"ubyte", "sbyte", "ushort", "sshort"} & set(loads), (name, loads)
        assert re.search(r"^\s*ds_read_b128\b", k["body"], re.M), name
        assert k["occupancy"] >= 4, (name, k["vgprs"])
