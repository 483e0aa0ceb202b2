"""What the compiler made of the kernels of kmpgpu_load_streams_ordered (no GPU needed: hipcc cross-compiles gfx950).

The gather is kmp_stream_gather_kernel with a fetch that starts inside a member.  It has to stay what that one is: ALIGNED 16-byte loads of
arena bytes and a byte funnel shift in registers, 16-byte stores only, no scratch, no LDS, and no fewer wavefronts per SIMD than the
capture-order gather has -- that floor is read from kmp_streams.hip's ISA here, not written down."""
import os
import re

import pytest

from test_packets_isa import CSRC, HIPCC, _isa


@pytest.fixture(scope="module")
def seq_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _isa("kmp_streams_seq.hip", str(tmp_path_factory.mktemp("isa")))


@pytest.fixture(scope="module")
def capture_gather(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    ks = {n: k for n, k in _isa("kmp_streams.hip", str(tmp_path_factory.mktemp("isa"))).items() if "kmp_stream_gather_kernel" in n}
    assert len(ks) == 2
    return ks


def test_the_file_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_streams_seq.hip" in hipsrc.split()


def test_gather_kernel(seq_isa, capture_gather):
    ks = {n: k for n, k in seq_isa.items() if "kmp_sseq_gather_kernel" in n}
    assert len(ks) == 2, [n for n in seq_isa if "sseq" in n]     # with and without the non-temporal hint
    floor = min(k["occupancy"] for k in capture_gather.values())
    for name, k in ks.items():
        assert k["scratch"] == 0 and "movrel" not in k["body"], name
        assert not re.search(r"^\s*ds_", k["body"], re.M), name                # no LDS
        loads = re.findall(r"^\s*(?:global|buffer|flat)_load_(\w+)", k["body"], re.M)
        stores = re.findall(r"^\s*(?:global|buffer|flat)_store_(\w+)", k["body"], re.M)
        # narrower than 16 bytes are the index records only: piece_dst[] (dwordx2); no byte or short load of anything
        assert set(loads) <= {"dwordx4", "dwordx3", "dwordx2"}, (name, loads)
        assert loads.count("dwordx4") >= 3, (name, loads)       # the piece record and one or two aligned units
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        assert re.search(r"^\s*v_alignbyte_b32\b", k["body"], re.M), name
        assert k["occupancy"] >= floor, (name, k["vgprs"], floor)
    nt = {n: bool(re.search(r"^\s*global_(?:load|store)_dwordx4 .* nt\b", k["body"], re.M)) for n, k in ks.items()}
    assert sorted(nt.values()) == [False, True], nt             # one instantiation carries the hint, the other does not


def test_index_kernels(seq_isa):
    for kernel in ("kmp_sseq_heads_kernel", "kmp_sseq_keys_kernel", "kmp_sseq_max_scan_kernel", "kmp_sseq_max_totals_kernel",
                   "kmp_sseq_take_scan_kernel", "kmp_sseq_take_totals_kernel", "kmp_sseq_records_kernel", "kmp_sseq_index_kernel"):
        ks = [k for n, k in seq_isa.items() if kernel in n]
        assert len(ks) == 1, (kernel, [n for n in seq_isa if "sseq" in n])
        assert ks[0]["scratch"] == 0 and "movrel" not in ks[0]["body"], kernel
        assert not re.search(r"_atomic_", ks[0]["body"]), kernel            # no atomic decides a value
