"""What the compiler made of the whole-payload kernels (KMPGPU_OPT_WHOLE_PAYLOAD; no GPU needed: hipcc cross-compiles gfx950).

Every whole-payload kernel has a default twin -- the same template arguments under the name without "_whole" -- and does a subset
of its work: no 0x00 test, no `dead` carry, no nul_limit.  So it must not be the larger or the slower-shaped of the two: no scratch
(the classed fused kernel included: its twin's spilled lane masks belong to the segmented strlen path), no run-time register
indexing, the twin's ring (hand-counted waits, buffer-load issues), at least the twin's occupancy, and for the counting kernels no
more instructions than the twin has."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multithreading_string_matching_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _isa(src, tmp):
    out = os.path.join(tmp, src + ".s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1048576",      # as csrc/Makefile
                        f"-I{ROOT}/include", f"-I{CSRC}", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
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
    return {src: _isa(src, tmp) for src in ("kmp_scan_stream.hip", "kmp_scan_multi.hip")}


def _ring_waits(body):
    """hand-written waits only (they sit between ;;#ASMSTART / ;;#ASMEND), by their count"""
    out = {}
    for n in re.findall(r";;#ASMSTART\s*\n\s*s_waitcnt vmcnt\((\d+)\)\s*\n\s*;;#ASMEND", body):
        out[int(n)] = out.get(int(n), 0) + 1
    return out


def _issues(body):
    return len(re.findall(r";;#ASMSTART\s*\n(?:\s*s_nop 4\s*\n)?\s*buffer_load_dwordx4 ", body))


def _instructions(body):
    n = 0
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if line and not line.endswith(":") and not line.startswith("."):
            n += 1
    return n


def _twin(name):
    """the mangled name of the default kernel with the same template arguments: <length><identifier without _whole>"""
    m = re.search(r"(kmp_scan_[a-z_]*?_whole[a-z_]*?_kernel)I", name)
    assert m, name
    whole = m.group(1)
    ident = whole.replace("_whole", "")
    assert "%d%sI" % (len(whole), whole) in name, name
    return name.replace("%d%sI" % (len(whole), whole), "%d%sI" % (len(ident), ident))


def _pairs(isa, src):
    ks = isa[src]
    whole = {n: k for n, k in ks.items() if "_whole" in n}
    for n in whole:
        assert _twin(n) in ks, (n, _twin(n))
    return [(n, k, ks[_twin(n)]) for n, k in sorted(whole.items())]


def _is_emit(name):
    return "whole_emit_kernel" in name or (re.search(r"kmp_scan_(flat|packed)_whole_kernel", name) is not None and "ELb1EEEv" in name)


def test_whole_kernels_exist_in_every_streaming_family(isa):
    stream = [n for n in isa["kmp_scan_stream.hip"] if "_whole" in n]
    multi = [n for n in isa["kmp_scan_multi.hip"] if "_whole" in n]
    for ident in ("kmp_scan_flat_whole_kernel", "kmp_scan_packed_whole_kernel"):
        assert [n for n in stream if ident in n and not _is_emit(n)], (ident, stream)             # counting
        assert len([n for n in stream if ident in n and _is_emit(n)]) == 1, (ident, stream)       # offset records / hit bitmap
    for ident in ("kmp_scan_multi_whole_kernel", "kmp_scan_multi_whole_wide_kernel", "kmp_scan_multi_whole_emit_kernel"):
        assert [n for n in multi if ident in n], (ident, multi)
    # the fused pass: plain and classed (last template argument) forms of all three entry points
    for ident in ("kmp_scan_multi_whole_kernel", "kmp_scan_multi_whole_wide_kernel", "kmp_scan_multi_whole_emit_kernel"):
        for classed in ("ELb0EEEv", "ELb1EEEv"):
            assert [n for n in multi if ident in n and classed in n], (ident, classed)
    # as many whole kernels as the fused pass has default ones: the dispatch picks a twin for every case
    assert len(multi) == len([n for n in isa["kmp_scan_multi.hip"] if "_whole" not in n and "kmp_scan_multi" in n])


@pytest.mark.parametrize("src", ["kmp_scan_stream.hip", "kmp_scan_multi.hip"])
def test_no_scratch_no_movrel_and_the_twins_ring(isa, src):
    pairs = _pairs(isa, src)
    assert pairs
    for name, k, twin in pairs:
        assert k["scratch"] == 0, name
        assert "movrel" not in k["body"], name
        assert _ring_waits(k["body"]) == _ring_waits(twin["body"]), name
        assert _issues(k["body"]) == _issues(twin["body"]) and _issues(k["body"]) > 0, name
        assert k["occupancy"] >= twin["occupancy"], (name, k["vgprs"], twin["vgprs"])


@pytest.mark.parametrize("src", ["kmp_scan_stream.hip", "kmp_scan_multi.hip"])
def test_counting_kernels_are_no_larger_than_their_twins(isa, src):
    counted = 0
    for name, k, twin in _pairs(isa, src):
        if _is_emit(name):
            continue
        print(name, _instructions(k["body"]), _instructions(twin["body"]), k["vgprs"], twin["vgprs"])
        assert _instructions(k["body"]) <= _instructions(twin["body"]), name
        counted += 1
    assert counted >= (4 if src == "kmp_scan_stream.hip" else 12)


def test_whole_kernels_test_no_byte_for_zero(isa):
    """The has-zero trick, (x - 0x01010101) & ~x & 0x80808080, is the strlen machinery itself: the default flat and packed kernels
    carry its constant, their whole-payload twins do not."""
    for name, k, twin in _pairs(isa, "kmp_scan_stream.hip"):
        if _is_emit(name):
            continue
        assert "0xfefefeff" in twin["body"], name
        assert "0xfefefeff" not in k["body"], name
