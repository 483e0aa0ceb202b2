"""What the compiler made of the kernels of kmpgpu_load_decoded (no GPU needed: hipcc cross-compiles gfx950).

kmp_decode.hip reads every payload byte in 16-byte loads, several units in flight per lane, and writes the decoded arena in whole
16-byte stores only -- compacted bytes are staged through the wavefront's LDS --, without scratch or run-time register indexing, at an
occupancy that hides the latency of the loads.  What the write kernel reads besides payload bytes is the index: the new offsets (8
bytes each) and the 16-byte records kmp_decode_index_kernel writes for it."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def decode_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_decode.hip", str(tmp_path_factory.mktemp("isa")))


def test_decode_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_decode.hip" in hipsrc.split()


def test_write_kernel(decode_isa):
    ks = {n: k for n, k in decode_isa.items() if "kmp_decode_write_kernel" in n}
    assert len(ks) == 2, list(decode_isa)                       # with and without the non-temporal hint
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        # payload bytes: dwordx4, four units in flight per lane; the index: offsets (dwordx2) and records (dwordx4, or the words used)
        assert set(loads) <= {"dwordx4", "dwordx3", "dwordx2"}, (name, loads)
        assert loads.count("dwordx4") >= 4, (name, loads)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert k["occupancy"] >= 4, (name, k["vgprs"])
    nt = {n: bool(re.search(r"^\s*global_(?:load|store)_dwordx4 .* nt\b", k["body"], re.M)) for n, k in ks.items()}
    assert sorted(nt.values()) == [False, True], nt             # one instantiation carries the hint, the other does not


def test_lengths_kernel(decode_isa):
    ks = [k for n, k in decode_isa.items() if "kmp_decode_lengths_kernel" in n]
    assert len(ks) == 1, list(decode_isa)
    k = ks[0]
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
    stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
    assert loads.count("dwordx4") >= 4, loads                   # payload bytes, four units in flight per lane
    assert stores and not set(stores) & {"byte", "short", "short_d16_hi", "byte_d16_hi"}, stores
    assert k["occupancy"] >= 4, k["vgprs"]
