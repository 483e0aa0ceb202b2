"""The host side of kmpgpu_scan_alerts (no GPU needed): the record's layout, the family names, the header's constants, the build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from multithreading_string_matching_amd import _lib, matcher
from multithreading_string_matching_amd.matcher import ALERT_DTYPE, ALERT_FAMILIES, GpuMatcher


def test_record_layout():
    """kmpgpu_alert: uint64 packet, uint32 index, uint32 reserved -- 16 bytes, as the kernel stores them"""
    assert ALERT_DTYPE.itemsize == 16 == C.sizeof(_lib.Alert)
    assert [(n, ALERT_DTYPE.fields[n][0].str, ALERT_DTYPE.fields[n][1]) for n in ALERT_DTYPE.names] == \
        [("packet", "<u8", 0), ("index", "<u4", 8), ("reserved", "<u4", 12)]
    assert [(n, getattr(_lib.Alert, n).offset, getattr(_lib.Alert, n).size) for n, _ in _lib.Alert._fields_] == \
        [("packet", 0, 8), ("index", 8, 4), ("reserved", 12, 4)]
    a = (_lib.Alert * 2)()
    a[1].packet, a[1].index = (1 << 40) + 5, 7
    rec = np.frombuffer(a, dtype=ALERT_DTYPE)
    assert int(rec[1]["packet"]) == (1 << 40) + 5 and int(rec[1]["index"]) == 7 and int(rec[1]["reserved"]) == 0


def test_constants_equal_the_header():
    text = open(os.path.join(ROOT, "include", "kmpgpu.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define KMPGPU_ALERT_(\w+)\s+(\d+)", text, re.M)}
    assert header == {"PATTERNS": 0, "RULES": 1, "RELATIONS": 2, "CHAINS": 3}
    for name, value in header.items():
        assert getattr(matcher, "ALERT_" + name) == value
        assert ALERT_FAMILIES[name.lower()] == value
    assert sorted(ALERT_FAMILIES) == ["chains", "patterns", "relations", "rules"]
    assert re.search(r"typedef struct kmpgpu_alert \{\s*uint64_t packet;.*?uint32_t index;.*?uint32_t reserved;", text, re.S)


def test_symbols_are_bound():
    for name in ("kmpgpu_scan_alerts", "kmpgpu_alerts_read"):
        assert name in _lib.GPU_API
        assert re.search(rf"\b{name}\(", open(os.path.join(ROOT, "include", "kmpgpu.h")).read())


def test_unknown_family_raises_before_any_gpu_call():
    m = object.__new__(GpuMatcher)                     # no context, no library: a GPU call would fail on the missing attributes
    for family in ("rule", "", None, 1):
        with pytest.raises(ValueError):
            GpuMatcher.scan_alerts(m, family)
    with pytest.raises(ValueError):
        GpuMatcher.scan_alerts(m, "rules", max_records=-1)


def test_alerts_kernels_are_in_the_build():
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        hipsrc = next(line for line in f if line.startswith("HIPSRC"))
    assert "kmp_alerts.hip" in hipsrc.split()
