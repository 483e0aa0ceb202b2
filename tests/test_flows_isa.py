"""What the compiler made of the flow kernels (no GPU needed: hipcc cross-compiles gfx950).

kmp_flows.hip: a lane per payload, its 16 bytes of metadata in one load, every atomic once per distinct target of the wavefront -- no
scratch, no run-time register indexing, and registers for at least the occupancy the rules kernel is held to."""
import os
import re

import pytest

from test_packets_isa import ATOMIC_OR_64, CSRC, HIPCC, _isa

KERNELS = ("kmp_flows_insert_kernel", "kmp_flows_firsts_kernel", "kmp_flows_number_kernel", "kmp_flows_assign_kernel", "kmp_flows_fold_kernel",
           "kmp_flows_expand_kernel")
GLOBAL_WRITE = re.compile(r"^\s*((?:global|buffer|flat|scratch)_(?:store|atomic)_\w+)", re.M)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_flows.hip", str(tmp_path_factory.mktemp("isa")))


def _kernel(isa, name):
    ks = [k for n, k in isa.items() if name in n]
    assert len(ks) == 1, list(isa)
    return ks[0]


def test_flow_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_flows.hip" in hipsrc.split()


def test_every_kernel_without_scratch_and_at_the_rules_kernels_occupancy(isa):
    assert len(isa) == len(KERNELS), list(isa)
    for name in KERNELS:
        k = _kernel(isa, name)
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        assert k["occupancy"] >= 4, (name, k["vgprs"])            # (what tests/test_rules_isa.py asks of the rules kernel)


def test_insert_kernel(isa):
    k = _kernel(isa, "kmp_flows_insert_kernel")
    loads = re.findall(r"^\s*(?:global|buffer)_load_(\w+)", k["body"], re.M)
    # the payload's record and the record of the payload a taken slot names: 16-byte loads; the slot itself one dword
    assert loads.count("dwordx4") == 2 and set(loads) == {"dwordx4", "dword"}, loads
    writes = GLOBAL_WRITE.findall(k["body"])
    # the compare-and-swap on a slot read as empty, slot_of, and the minimum: one of each, the minimum behind the ballot loop
    assert sorted(writes) == ["global_atomic_cmpswap", "global_atomic_umin", "global_store_dword"], writes
    assert "v_readlane_b32" in k["body"]


def test_assign_kernel_adds_once_per_flow_of_the_wavefront(isa):
    k = _kernel(isa, "kmp_flows_assign_kernel")
    writes = GLOBAL_WRITE.findall(k["body"])
    assert sorted(writes) == ["global_atomic_add_x2", "global_atomic_add_x2", "global_atomic_umax_x2", "global_store_dword"], writes
    assert "v_readlane_b32" in k["body"]


def test_fold_kernel_writes_with_the_atomic_or_alone(isa):
    k = _kernel(isa, "kmp_flows_fold_kernel")
    writes = GLOBAL_WRITE.findall(k["body"])
    assert writes == ["global_atomic_or_x2"], writes
    assert ATOMIC_OR_64.search(k["body"])
    # flow_of: one dword per lane, once; nothing else comes through the vector memory path
    loads = re.findall(r"^\s*(?:global|buffer)_load_(\w+)", k["body"], re.M)
    assert loads == ["dword"], loads


def test_expand_kernel_stores_a_word_per_wavefront(isa):
    k = _kernel(isa, "kmp_flows_expand_kernel")
    assert GLOBAL_WRITE.findall(k["body"]) == ["global_store_dwordx2"]
