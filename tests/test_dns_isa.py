"""What the compiler made of the kernels of kmpgpu_dns_locate / kmpgpu_load_dns (no GPU needed: hipcc cross-compiles gfx950).

The locate's walk holds one 16-byte unit in registers and takes a length byte out of it with selects and shifts, and it sets a bit
of a 256-bit mask kept in eight registers: neither may turn into run-time register indexing or scratch.  Every payload byte is read
in 16-byte loads.  Its latency is hidden by the number of wavefronts alone -- a lane waits for the unit it asked for before it knows
where the next length byte lies -- so the occupancy of 8 is what its speed rests on."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa

KERNELS = ["kmp_dns_gather_kernel", "kmp_dns_gather_kernel", "kmp_dns_index_kernel", "kmp_dns_lengths_kernel", "kmp_dns_locate_kernel",
           "kmp_dns_locate_kernel"]


@pytest.fixture(scope="module")
def dns_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_dns.hip", str(tmp_path_factory.mktemp("isa")))


def test_dns_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_dns.hip" in hipsrc.split()


def test_the_file_holds_these_kernels_only(dns_isa):
    """the scan kernels are the ones of kmp_prep.hip, not copies; the locate has one instantiation per prefix, the gather one per hint"""
    names = sorted(next((s for s in set(KERNELS) if s in n), n) for n in dns_isa)
    assert names == KERNELS, list(dns_isa)


def test_no_scratch_and_no_register_indexing(dns_isa):
    for name, k in dns_isa.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name


def test_locate_kernel(dns_isa):
    ks = {n: k for n, k in dns_isa.items() if "kmp_dns_locate_kernel" in n}
    assert len(ks) == 2, list(dns_isa)
    for name, k in ks.items():
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        # payload bytes: whole units; the index: offsets (dwordx2) and lengths (dword)
        assert "dwordx4" in loads and set(loads) <= {"dwordx4", "dwordx2", "dword"}, (name, loads)
        assert k["occupancy"] == 8, (name, k["vgprs"])


def test_gather_kernel(dns_isa):
    ks = {n: k for n, k in dns_isa.items() if "kmp_dns_gather_kernel" in n}
    assert len(ks) == 2, list(dns_isa)                          # with and without the non-temporal hint
    for name, k in ks.items():
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert k["occupancy"] == 8, (name, k["vgprs"])
