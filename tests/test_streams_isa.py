"""What the compiler made of the kernels of kmpgpu_load_streams (no GPU needed: hipcc cross-compiles gfx950).

The gather builds a 16-byte destination unit from any number of pieces, none of them 16-byte aligned relative to it.  It must do so with
ALIGNED 16-byte loads and a byte funnel shift in registers: a byte, word or dword load of arena bytes would be an unaligned walk over
the source, and it is the aligned loads that keep every read inside a member's slot.  What the kernel reads besides arena bytes is the
index: the pieces' destination addresses (8 bytes each) and their 16-byte records.  This file looks at load widths and register
pressure, nothing else."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def streams_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_streams.hip", str(tmp_path_factory.mktemp("isa")))


def test_stream_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_streams.hip" in hipsrc.split()


def test_gather_kernel(streams_isa):
    ks = {n: k for n, k in streams_isa.items() if "kmp_stream_gather_kernel" in n}
    assert len(ks) == 2, list(streams_isa)                      # with and without the non-temporal hint
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        # narrower than 16 bytes are the index records only: piece_dst[] (dwordx2) and the three words read of a piece's record (dwordx3)
        assert set(loads) <= {"dwordx4", "dwordx3", "dwordx2"}, (name, loads)
        assert loads.count("dwordx4") >= 2 and loads.count("dwordx3") + loads.count("dwordx4") >= 3, (name, loads)     # one or two aligned units
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert re.search(r"^\s*v_alignbyte_b32\b", k["body"], re.M), name
        assert k["occupancy"] >= 4, (name, k["vgprs"])
    nt = {n: bool(re.search(r"^\s*global_(?:load|store)_dwordx4 .* nt\b", k["body"], re.M)) for n, k in ks.items()}
    assert sorted(nt.values()) == [False, True], nt             # one instantiation carries the hint, the other does not


def test_index_kernels(streams_isa):
    for kernel in ("kmp_stream_scan_kernel", "kmp_stream_totals_kernel", "kmp_stream_heads_kernel", "kmp_stream_records_kernel",
                   "kmp_stream_index_kernel"):
        ks = [k for n, k in streams_isa.items() if kernel in n]
        assert len(ks) == 1, (kernel, list(streams_isa))
        assert ks[0]["scratch"] == 0 and "movrel" not in ks[0]["body"], kernel
        assert not re.search(r"_atomic_", ks[0]["body"]), kernel            # no atomic decides a value
