"""What the compiler made of the kernels of kmpgpu_load_base64 (no GPU needed: hipcc cross-compiles gfx950).

kmp_base64.hip follows kmp_decode.hip: every payload byte is read in 16-byte loads, several units in flight per lane -- the look-ahead
behind a step's last unit too --, the decoded arena goes out in whole 16-byte stores only, compacted bytes are staged through the
wavefront's LDS, and there is no scratch and no run-time register indexing.  What the write kernel reads besides payload bytes is the
index: the new offsets (8 bytes each) and the 16-byte records kmp_decode_index_kernel writes for it.  The occupancies and the counts of
16-byte loads are the ones the ISA shows (116 VGPRs in the lengths kernel, 96 in the write kernel; eight and nine loads: four of units, four look-aheads, one per
step of the unroll, and the write's records): a change that costs a wave per SIMD, or narrows or adds a load, shows here."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def base64_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_base64.hip", str(tmp_path_factory.mktemp("isa")))


def test_base64_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_base64.hip" in hipsrc.split()


def test_the_file_holds_these_kernels_only(base64_isa):
    """the scan and the index kernels are the ones of kmp_prep.hip and kmp_decode.hip, not copies"""
    names = sorted(next((s for s in ("kmp_base64_lengths_kernel", "kmp_base64_write_kernel") if s in n), n) for n in base64_isa)
    assert names == ["kmp_base64_lengths_kernel", "kmp_base64_write_kernel", "kmp_base64_write_kernel"], list(base64_isa)


def test_write_kernel(base64_isa):
    ks = {n: k for n, k in base64_isa.items() if "kmp_base64_write_kernel" in n}
    assert len(ks) == 2, list(base64_isa)                       # with and without the non-temporal hint
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        # payload bytes: dwordx4, four units in flight per lane; the index: offsets (dwordx2) and records (dwordx4, or the words used)
        assert set(loads) <= {"dwordx4", "dwordx3", "dwordx2"}, (name, loads)
        assert loads.count("dwordx4") == 9, (name, loads)          # four units, four look-aheads, the records
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert k["occupancy"] == 5, (name, k["vgprs"])
    nt = {n: bool(re.search(r"^\s*global_(?:load|store)_dwordx4 .* nt\b", k["body"], re.M)) for n, k in ks.items()}
    assert sorted(nt.values()) == [False, True], nt             # one instantiation carries the hint, the other does not


def test_look_ahead_loads(base64_isa):
    """the load that decides a run which leaves a step undecided is written as a volatile access, so it carries sc0 sc1: a whole 16-byte
    load, once per step of the 4-unit unroll, in every kernel -- beside the four loads of the units themselves"""
    for name, k in base64_isa.items():
        vol = re.findall(r"^\s*global_load_(\w+) .*\bsc0 sc1\b", k["body"], re.M)
        assert vol == ["dwordx4"] * 4, (name, vol)


def test_lengths_kernel(base64_isa):
    ks = [k for n, k in base64_isa.items() if "kmp_base64_lengths_kernel" in n]
    assert len(ks) == 1, list(base64_isa)
    k = ks[0]
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
    stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
    assert loads.count("dwordx4") == 8, loads                   # payload bytes: four units in flight per lane, a look-ahead per step of the unroll
    assert set(loads) <= {"dwordx4", "dwordx2", "dword"}, loads  # ... and the index: offsets and lengths
    assert stores and not set(stores) & {"byte", "short", "short_d16_hi", "byte_d16_hi"}, stores
    assert k["occupancy"] == 4, k["vgprs"]
