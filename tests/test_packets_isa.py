"""What the compiler made of kmpgpu_scan_packets on the device (no GPU needed: hipcc cross-compiles gfx950).

The scan kernels that emit matches (the EMIT instantiations of kmp_scan_stream.hip and kmp_scan_multi.hip) also mark the
hit matrix, with a 64-bit atomic OR per distinct (pattern, packet) pair; the count-only kernels must not carry one.  The
reduce over the matrix (kmp_marks.hip) reads it with 16-byte loads, without scratch or run-time register indexing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ATOMIC_OR_64 = re.compile(r"^\s*(global|buffer|flat)_atomic_or_x2\b", re.M)


def _isa(src, tmp):
    path = os.path.join(CSRC, src)
    assert os.path.exists(path), f"csrc/{src} is missing"
    out = os.path.join(tmp, src + ".s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1048576",      # as csrc/Makefile
                        f"-I{ROOT}/include", f"-I{CSRC}", "-S", "--cuda-device-only", "-o", out, path],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\.Lfunc_end\d+:.*?^; NumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; Occupancy: (\d+)",
                         text, re.S | re.M):
        # (the whole kernel, every path to its s_endpgm)
        kernels[m.group(1)] = {"body": m.group(2), "vgprs": int(m.group(3)), "scratch": int(m.group(4)), "occupancy": int(m.group(5))}
    return kernels


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = str(tmp_path_factory.mktemp("isa"))
    return {src: _isa(src, tmp) for src in ("kmp_marks.hip", "kmp_scan_stream.hip", "kmp_scan_multi.hip")}


def test_marks_reduce_is_in_the_build():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_marks.hip" in hipsrc.split()


def test_marks_reduce_kernel(isa):
    ks = {n: k for n, k in isa["kmp_marks.hip"].items() if "kmp_marks_reduce_kernel" in n}
    assert len(ks) == 1, list(isa["kmp_marks.hip"])
    k = next(iter(ks.values()))
    assert k["scratch"] == 0 and "movrel" not in k["body"]
    loads = re.findall(r"^\s*(?:global|buffer)_load_(\w+)", k["body"], re.M)
    # the matrix is read in 16-byte loads, several of them in flight per lane
    assert loads and set(loads) == {"dwordx4"}, loads
    assert len(loads) >= 4
    assert k["occupancy"] >= 4, k["vgprs"]


def _emit_kernels(isa):
    stream = {n: k for n, k in isa["kmp_scan_stream.hip"].items()
              if ("kmp_scan_flat_kernelILi4E" in n or "kmp_scan_packed_kernelILi4E" in n) and "ELb1EEEv" in n}
    fused = {n: k for n, k in isa["kmp_scan_multi.hip"].items() if "kmp_scan_multi_emit_kernel" in n}
    return stream, fused


def test_emit_kernels_mark_with_a_64_bit_atomic_or(isa):
    stream, fused = _emit_kernels(isa)
    assert len(stream) == 2 and len(fused) >= 4, (list(stream), list(fused))
    for name, k in list(stream.items()) + list(fused.items()):
        assert ATOMIC_OR_64.search(k["body"]), name
        assert k["scratch"] == 0, name
    for name, k in fused.items():
        assert k["occupancy"] >= 4, (name, k["vgprs"])


def test_count_kernels_carry_no_atomic_or(isa):
    stream, fused = _emit_kernels(isa)
    emit = set(stream) | set(fused)
    counted = 0
    for src in ("kmp_scan_stream.hip", "kmp_scan_multi.hip"):
        for name, k in isa[src].items():
            if name in emit or not re.search(r"kmp_scan_(flat|packed|multi|multi_wide)_kernel", name):
                continue
            assert not ATOMIC_OR_64.search(k["body"]), name
            counted += 1
    assert counted >= 30
