"""What the compiler made of the chain kernel of kmpgpu_scan_chains (no GPU needed: hipcc cross-compiles gfx950).

One kernel (kmp_chains.hip): a wavefront per (chain, 64 payloads), a sweep over a candidate payload with one carry per link kept in
the lanes of a register -- no scratch, no run-time register indexing, and registers for at least four wavefronts per SIMD."""
import os

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_chains.hip", str(tmp_path_factory.mktemp("isa")))


def test_chains_kernel_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_chains.hip" in hipsrc.split()


def test_chains_kernel(isa):
    ks = {n: k for n, k in isa.items() if "kmp_chains_kernel" in n}
    assert len(ks) == 1 and len(isa) == 1, list(isa)
    k = next(iter(ks.values()))
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    assert k["occupancy"] >= 4, k["vgprs"]
