"""What the compiler made of the kernels of kmpgpu_load_selected (no GPU needed: hipcc cross-compiles gfx950).

kmp_select.hip moves every payload byte in 16-byte loads and 16-byte stores (source and destination slots are 16-byte aligned),
several units in flight per lane, without scratch or run-time register indexing, at an occupancy that hides the latency of the
loads.  What the copy kernel reads besides payload bytes is the index: the new offsets (8 bytes each) and the 16-byte records
{source offset, length} that kmp_select_index_kernel writes for it -- so no load of the kernel is narrower than 8 bytes (a byte
or dword load would be one of payload bytes) and no store is anything but 16."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def select_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_select.hip", str(tmp_path_factory.mktemp("isa")))


def test_select_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_select.hip" in hipsrc.split()


def test_copy_kernel(select_isa):
    ks = {n: k for n, k in select_isa.items() if "kmp_select_copy_kernel" in n}
    assert len(ks) == 2, list(select_isa)                       # with and without the non-temporal hint
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        # payload bytes: dwordx4 both ways, four units in flight per lane; the index: offsets (dwordx2) and records (three words
        # of the 16-byte record are used, so the compiler may read just those)
        assert set(loads) <= {"dwordx4", "dwordx3", "dwordx2"}, (name, loads)
        assert loads.count("dwordx4") >= 4, (name, loads)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert len(stores) >= 4, (name, stores)
        assert k["occupancy"] >= 4, (name, k["vgprs"])
    nt = {n: bool(re.search(r"^\s*global_(?:load|store)_dwordx4 .* nt\b", k["body"], re.M)) for n, k in ks.items()}
    assert sorted(nt.values()) == [False, True], nt             # one instantiation carries the hint, the other does not


def test_index_kernels(select_isa):
    for kernel in ("kmp_select_lengths_kernel", "kmp_select_index_kernel"):
        ks = [k for n, k in select_isa.items() if kernel in n]
        assert len(ks) == 1, (kernel, list(select_isa))
        assert ks[0]["scratch"] == 0 and "movrel" not in ks[0]["body"], kernel
    # the record the copy reads is written whole
    k = next(k for n, k in select_isa.items() if "kmp_select_index_kernel" in n)
    assert re.search(r"^\s*global_store_dwordx4\b", k["body"], re.M)
