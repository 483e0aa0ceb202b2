"""What the compiler made of the regex kernel of kmpgpu_scan_regexes (no GPU needed: hipcc cross-compiles gfx950).

kmp_regex.hip: a lane per payload, KMP_RX_TILE expressions out of LDS with their reach sets in registers, the text in 16-byte loads, the
rows written in 16-byte pieces -- in its two instantiations (strlen rule, whole payloads).  No scratch, no run-time register indexing,
and registers for at least the occupancy the rules kernel is held to."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_regex.hip", str(tmp_path_factory.mktemp("isa")))


def test_regex_kernel_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC")).split()
    assert "kmp_regex.hip" in hipsrc and "kmp_regex.cpp" in hipsrc


def test_the_file_holds_two_instantiations(isa):
    assert len(isa) == 2, list(isa)
    assert all("kmp_regex_kernel" in n for n in isa)
    assert sum("ILb1E" in n for n in isa) == 1 and sum("ILb0E" in n for n in isa) == 1


def test_regex_kernels(isa):
    for name, k in isa.items():
        # the reach sets of a tile stay in registers
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        # a row leaves in 16-byte pieces, and nothing else is stored
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        # the text and the table come in 16-byte loads, never byte by byte
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        assert "dwordx4" in loads and not {"ubyte", "sbyte", "ushort", "sshort"} & set(loads), (name, loads)
        # the tile's words of one text byte come out of LDS 16 bytes at a time
        assert re.search(r"^\s*ds_read_b128\b", k["body"], re.M), name
        assert k["occupancy"] >= 4, (name, k["vgprs"])     # (what tests/test_rules_isa.py asks of the rules kernel)
