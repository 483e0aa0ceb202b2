"""What the compiler made of the threshold kernels (no GPU needed: hipcc cross-compiles gfx950).

kmp_thresholds.hip: in the build; no kernel spills; the scan kernels -- reduce and scan, of 64-bit maxima and of 32-bit sums -- and the
gather read and write 16 bytes a lane; every kernel leaves room for four wavefronts per SIMD and more."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_thresholds.hip", str(tmp_path_factory.mktemp("isa")))


def test_the_file_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC")).split()
    assert "kmp_thresholds.hip" in hipsrc and "kmp_flowbits.hip" in hipsrc


def test_no_scratch_and_occupancy(isa):
    names = " ".join(isa)
    for stem in ("kmp_thr_reduce_kernel", "kmp_thr_scan_kernel", "kmp_thr_keys_kernel", "kmp_thr_tsort_kernel", "kmp_thr_gather_kernel",
                 "kmp_thr_pass_kernel", "kmp_thr_final_kernel"):
        assert stem in names, stem
    assert sum("kmp_thr_reduce_kernel" in n for n in isa) == 2 and sum("kmp_thr_scan_kernel" in n for n in isa) == 4
    assert sum("kmp_thr_pass_kernel" in n for n in isa) == 2
    for name, k in isa.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        assert k["occupancy"] >= 4, (name, k["vgprs"])


def test_the_scan_kernels_move_16_bytes_a_lane(isa):
    for name, k in isa.items():
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        if "kmp_thr_reduce_kernel" in name:
            assert "dwordx4" in loads, (name, loads)
        if "kmp_thr_scan_kernel" in name or "kmp_thr_gather_kernel" in name:
            assert "dwordx4" in loads and "dwordx4" in stores, (name, loads, stores)
