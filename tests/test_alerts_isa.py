"""What the compiler made of the list kernels of kmpgpu_scan_alerts (no GPU needed: hipcc cross-compiles gfx950).

kmp_alerts.hip walks the rows of a family twice: kmp_alerts_count_kernel counts the set bits of every column, kmp_alerts_fill_kernel
writes one 16-byte record per set bit at the position the scan gave its payload.  Both read the rows in 16-byte loads, transpose in
registers (no scratch, no run-time register indexing), and no atomic decides where a record goes."""
import os
import re

import pytest

from test_packets_isa import HIPCC, _isa


@pytest.fixture(scope="module")
def alerts_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_alerts.hip", str(tmp_path_factory.mktemp("isa")))


def _one(alerts_isa, kernel):
    ks = [k for n, k in alerts_isa.items() if kernel in n]
    assert len(ks) == 1, (kernel, list(alerts_isa))
    return ks[0]


@pytest.mark.parametrize("kernel", ["kmp_alerts_count_kernel", "kmp_alerts_fill_kernel"])
def test_walk(alerts_isa, kernel):
    k = _one(alerts_isa, kernel)
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
    assert loads.count("dwordx4") >= 2, loads                   # 32 bytes of a row per lane
    assert not re.search(r"^\s*(?:global|buffer|flat)_atomic_", k["body"], re.M)
    assert k["occupancy"] >= 4, k["vgprs"]


def test_fill_writes_whole_records(alerts_isa):
    k = _one(alerts_isa, "kmp_alerts_fill_kernel")
    stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
    assert stores and set(stores) == {"dwordx4"}, stores


def test_count_writes_one_word_per_payload(alerts_isa):
    k = _one(alerts_isa, "kmp_alerts_count_kernel")
    stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
    assert stores and set(stores) == {"dword"}, stores
