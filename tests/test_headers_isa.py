"""What the compiler made of the header kernel of kmpgpu_scan_headers (no GPU needed: hipcc cross-compiles gfx950).

kmp_headers.hip: a lane per payload, its 16 bytes of metadata in one load, the predicates out of LDS, the rows written in 16-byte
pieces -- no scratch, no run-time register indexing, and registers for at least the occupancy the rules kernel is held to."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_headers.hip", str(tmp_path_factory.mktemp("isa")))


def test_headers_kernel_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_headers.hip" in hipsrc.split()


def test_headers_kernel(isa):
    ks = {n: k for n, k in isa.items() if "kmp_headers_kernel" in n}
    assert len(ks) == 1, list(isa)
    k = next(iter(ks.values()))
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    loads = re.findall(r"^\s*(?:global|buffer)_load_(\w+)", k["body"], re.M)
    # the metadata record and the predicates' records in 16-byte loads, the length as one dword: nothing narrower, nothing per byte
    assert loads.count("dwordx4") >= 2 and set(loads) == {"dwordx4", "dword"}, loads
    assert loads.count("dword") == 1, loads
    # a row leaves in 16-byte pieces
    stores = re.findall(r"^\s*(?:global|buffer)_store_(\w+)", k["body"], re.M)
    assert stores and set(stores) == {"dwordx4"}, stores
    assert k["occupancy"] >= 4, k["vgprs"]                # (what tests/test_rules_isa.py asks of the rules kernel)


def test_metadata_kernels(isa):
    """the two kernels that carry the metadata beside the index write a record in one 16-byte store, without scratch"""
    ks = {n: k for n, k in isa.items() if "kmp_meta_extract_kernel" in n or "kmp_meta_select_kernel" in n}
    assert len(ks) == 2 and len(isa) == 3, list(isa)
    for name, k in ks.items():
        assert k["scratch"] == 0, name
        stores = re.findall(r"^\s*(?:global|buffer)_store_(\w+)", k["body"], re.M)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
