"""What the compiler made of the fold kernel (kmp_fold.hip), the hot path of case-insensitive patterns.  No GPU needed:
hipcc cross-compiles gfx950.  The fold is a streaming read-modify-write at memory bandwidth: 128-bit vector loads and
stores, no scratch, no register reached through a run-time index."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def fold_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    src = os.path.join(CSRC, "kmp_fold.hip")
    assert os.path.exists(src), "csrc/kmp_fold.hip is missing"
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "kmp_fold.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1048576",      # as csrc/Makefile
                        f"-I{ROOT}/include", f"-I{CSRC}", "-S", "--cuda-device-only", "-o", out, src],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\s*s_endpgm\b(.*?)^; NumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; Occupancy: (\d+)", text, re.S | re.M):
        # (the whole kernel: the fold has more than one s_endpgm, one per path)
        kernels[m.group(1)] = {"body": m.group(2) + m.group(3), "vgprs": int(m.group(4)), "scratch": int(m.group(5)), "occupancy": int(m.group(6))}
    return kernels


def _fold_kernel(kernels):
    ks = {n: k for n, k in kernels.items() if "kmp_fold_kernel" in n}
    assert len(ks) == 1, list(kernels)
    return next(iter(ks.values()))


def test_fold_kernel_exists_without_scratch_or_movrel(fold_isa):
    for name, k in fold_isa.items():
        assert k["scratch"] == 0, name
        assert "movrel" not in k["body"], name
    k = _fold_kernel(fold_isa)
    assert k["occupancy"] >= 8, k["vgprs"]


def test_fold_kernel_moves_128_bit_vectors(fold_isa):
    body = _fold_kernel(fold_isa)["body"]
    loads = re.findall(r"^\s*(global|buffer)_load_(\w+)", body, re.M)
    stores = re.findall(r"^\s*(global|buffer)_store_(\w+)", body, re.M)
    assert loads and stores
    # every vector memory access of the kernel is a 16-byte one, with the non-temporal hint (each byte is touched once)
    assert {w for _, w in loads} == {"dwordx4"} and {w for _, w in stores} == {"dwordx4"}, (loads, stores)
    assert len(re.findall(r"_load_dwordx4 [^\n]*\bnt\b", body)) == len(loads)
    assert len(re.findall(r"_store_dwordx4 [^\n]*\bnt\b", body)) == len(stores)
    # several loads in flight per lane before the first store of the main path
    first_store = re.search(r"^\s*(global|buffer)_store_", body, re.M).start()
    assert len(re.findall(r"_load_dwordx4", body[:first_store])) >= 1
    assert len(re.findall(r"^\s*global_load_dwordx4", body, re.M)) >= 4


def test_fold_swar_is_exact():
    """The SWAR form of the kernel (kmp_fold.hip, fold4), evaluated on the host for every byte in every lane position."""
    def fold4(x):
        t = x & 0x7F7F7F7F
        up = (((t + 0x3F3F3F3F) ^ (t + 0x25252525)) & ~x & 0x80808080) & 0xFFFFFFFF
        return (x | (up >> 2)) & 0xFFFFFFFF
    for b in range(256):
        want = b + 0x20 if 0x41 <= b <= 0x5A else b
        for lane in range(4):
            for other in (0x00, 0x41, 0x5A, 0xC1, 0xFF):
                x = (b << (8 * lane)) | sum(other << (8 * j) for j in range(4) if j != lane)
                got = (fold4(x) >> (8 * lane)) & 0xFF
                assert got == want, (hex(b), lane, hex(other))
