"""What the compiler made of the kernels of kmpgpu_load_seams (no GPU needed: hipcc cross-compiles gfx950).

The gather builds a 16-byte destination unit from up to two pieces that are not 16-byte aligned relative to it.  It must do so with
ALIGNED 16-byte loads and a byte funnel shift in registers: a byte, word or dword load of arena bytes would be an unaligned walk
over the source, and it is the aligned loads that keep every read inside the slots of prev and next.  What the kernel reads besides
arena bytes is the index: the new offsets (8 bytes each) and the 16-byte halves of the records kmp_seam_index_kernel writes for it."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def seams_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_seams.hip", str(tmp_path_factory.mktemp("isa")))


def test_seam_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_seams.hip" in hipsrc.split()


def test_gather_kernel(seams_isa):
    ks = {n: k for n, k in seams_isa.items() if "kmp_seam_gather_kernel" in n}
    assert len(ks) == 2, list(seams_isa)                        # with and without the non-temporal hint
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        assert set(loads) <= {"dwordx4", "dwordx3", "dwordx2"}, (name, loads)
        assert loads.count("dwordx4") >= 4, (name, loads)       # two pieces of up to two aligned units each
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert re.search(r"^\s*v_alignbyte_b32\b", k["body"], re.M), name
        assert k["occupancy"] >= 4, (name, k["vgprs"])
    nt = {n: bool(re.search(r"^\s*global_(?:load|store)_dwordx4 .* nt\b", k["body"], re.M)) for n, k in ks.items()}
    assert sorted(nt.values()) == [False, True], nt             # one instantiation carries the hint, the other does not


def test_per_payload_kernels(seams_isa):
    for kernel in ("kmp_seam_keys_kernel", "kmp_seam_pred_kernel", "kmp_seam_index_kernel"):
        ks = [k for n, k in seams_isa.items() if kernel in n]
        assert len(ks) == 1, (kernel, list(seams_isa))
        assert ks[0]["scratch"] == 0 and "movrel" not in ks[0]["body"], kernel
        assert not re.search(r"_atomic_", ks[0]["body"]), kernel            # no atomic decides an order
    # the keys kernel takes a payload's record and its flow's first record in one 16-byte load each
    k = next(k for n, k in seams_isa.items() if "kmp_seam_keys_kernel" in n)
    assert len(re.findall(r"^\s*global_load_dwordx[34]\b", k["body"], re.M)) >= 2
