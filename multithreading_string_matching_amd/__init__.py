"""MI355X-native KMP packet-payload matcher -- the match-count hot path of
Lemnon95/multithreading_string_matching (serial.c:153-155, openmp_data.c:157-175) on gfx950.

Layout: ``csrc/`` holds the HIP kernels, the C-ABI (include/kmpgpu.h) and the C host side
(include/kmphost.h) with the two drop-in programs ``bin/serial`` and ``bin/openmp_data``; the
Python modules are thin ctypes views used by the tests, the benchmark and the smoke check.
"""
from ._lib import KmpGpuError, KmpHostError, SynthParams, build  # noqa: F401
from .host import (  # noqa: F401
    HostArena,
    arena_layout,
    extract,
    failure_table,
    format_report,
    load_patterns,
    parse_patterns,
    read_pcap,
    synth_count_planted,
    synth_fill_host,
    write_udp_pcap,
)
from .matcher import (  # noqa: F401
    B64_ONLY_CHANGED,
    B64_URLSAFE,
    DECODE_ONLY_CHANGED,
    DECODE_PERCENT,
    DECODE_PLUS,
    DNS_ONLY_PRESENT,
    DNS_QNAME,
    DNS_TCP_PREFIX,
    FIELD_BODY,
    FIELD_HEADERS,
    FIELD_METHOD,
    FIELD_RAW_URI,
    FIELD_STATUS,
    FIELDS_ONLY_PRESENT,
    GpuComm,
    GpuMatcher,
    LINK_BITMAP,
    LINK_INDEX,
    LINK_NONE,
    LINK_SAME,
    TLS_ALPN,
    TLS_ONLY_PRESENT,
    TLS_SNI,
    count_matches,
    device_count,
)
