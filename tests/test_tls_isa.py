"""What the compiler made of the kernels of kmpgpu_tls_locate / kmpgpu_load_tls (no GPU needed: hipcc cross-compiles gfx950).

The locate's walk holds one 16-byte unit in registers and takes a byte out of it with selects and shifts, and it sets a bit of a
256-bit mask kept in eight registers: neither may turn into run-time register indexing or scratch."""
import os

import pytest

from test_packets_isa import CSRC, HIPCC, _isa

KERNELS = ["kmp_tls_gather_kernel", "kmp_tls_gather_kernel", "kmp_tls_index_kernel", "kmp_tls_lengths_kernel", "kmp_tls_locate_kernel"]


@pytest.fixture(scope="module")
def tls_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_tls.hip", str(tmp_path_factory.mktemp("isa")))


def test_tls_kernels_are_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_tls.hip" in hipsrc.split()


def test_the_file_holds_these_kernels_only(tls_isa):
    """the scan kernels are the ones of kmp_prep.hip, not copies; one locate, one gather for both fields with one instantiation per hint"""
    names = sorted(next((s for s in set(KERNELS) if s in n), n) for n in tls_isa)
    assert names == KERNELS, list(tls_isa)


def test_no_scratch_and_no_register_indexing(tls_isa):
    for name, k in tls_isa.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
