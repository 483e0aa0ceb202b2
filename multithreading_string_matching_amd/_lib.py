"""ctypes bindings of the two product libraries.

* ``libkmphost.so`` -- plain C host side (include/kmphost.h): no GPU needed.
* ``libkmpgpu.so``  -- the gfx950 C-ABI (include/kmpgpu.h): the hot path.  There is no CPU
  fallback: every compute entry point raises ``KmpGpuError`` when the library, or a gfx950
  device, is missing.

Both are built in-tree by ``csrc/Makefile`` (``build()``), so the files travel with the repo.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
BINDIR = os.path.join(_HERE, "bin")
HOST_SO = os.path.join(LIBDIR, "libkmphost.so")
GPU_SO = os.path.join(LIBDIR, "libkmpgpu.so")

KMP_SYNTH_MAX_NEEDLE = 100
KMP_PCAP_ERRBUF = 256
KMP_RULES_ERRBUF = 256
KMP_WINDOWS_ERRBUF = 256
KMP_RELATIONS_ERRBUF = 256
KMP_CHAINS_ERRBUF = 256
KMP_HEADERS_ERRBUF = 256
HDR_ANY_PROTO, HDR_BIDIR = 1, 2   # KMPGPU_HDR_* / KMP_HDR_*: flags of a header predicate
HDR_TILE = 128             # KMP_HDR_TILE (csrc/kmp_launch.h): predicates the header kernel stages at a time
KMP_BYTETESTS_ERRBUF = 256
KMP_REGEXES_ERRBUF = 256
BT_RELATIVE, BT_LITTLE = 1, 2     # KMPGPU_BT_* / KMP_BT_*: flags of a byte test
BT_EQ, BT_NE, BT_LT, BT_GT, BT_LE, BT_GE = range(6)    # ... and its operators
BT_TILE = 128              # KMP_BT_TILE (csrc/kmp_launch.h): tests the absolute byte-test kernel stages at a time
RX_NOCASE, RX_DOTALL, RX_GATED = 1, 2, 4   # KMPGPU_RX_*: flags of an expression (kmpgpu_set_regexes)
RX_GROUPS = 16             # KMPGPU_RX_GROUPS: groups and alternation
RX_MAX_POSITIONS = 63      # KMPGPU_RX_MAX_POSITIONS
RX_MAX_EDGES = 8           # KMPGPU_RX_MAX_EDGES: edge rules of an expression under RX_GROUPS
RXG_TILE = 4               # KMP_RXG_TILE (csrc/kmp_regex.h): expressions the grouped regex kernel stages at a time
RX_TILE = 8                # KMP_RX_TILE (csrc/kmp_regex.h): expressions the regex kernel stages at a time
CHAIN_MAX = 8              # KMPGPU_CHAIN_MAX / KMP_CHAIN_MAX: contents of one chain
REL_NO_MIN = -(1 << 31)    # kmpgpu_relation.dmin == INT32_MIN: no lower bound
REL_NO_MAX = (1 << 31) - 1  # kmpgpu_relation.dmax == INT32_MAX: no upper bound
RULE_NOT = 0x80000000      # KMPGPU_RULE_NOT / KMP_RULE_NOT: the term's pattern must not be in the payload

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i32p = C.POINTER(C.c_int32)


class KmpGpuError(RuntimeError):
    pass


class KmpHostError(RuntimeError):
    pass


class SynthParams(C.Structure):
    """kmp_synth_params (include/kmp_synth.h)."""
    _fields_ = [
        ("seed", C.c_uint32), ("lo", C.c_uint32), ("span", C.c_uint32), ("plant_permille", C.c_uint32),
        ("nul_ppm", C.c_uint32), ("needle_len", C.c_uint32), ("needle", C.c_uint8 * KMP_SYNTH_MAX_NEEDLE),
    ]

    @classmethod
    def make(cls, seed=1234, needle=b"NEEDLE_16B_PATRN", plant_permille=100, nul_ppm=0, lo=ord("a"), span=26):
        p = cls()
        p.seed, p.lo, p.span, p.plant_permille, p.nul_ppm = seed, lo, span, plant_permille, nul_ppm
        p.needle_len = len(needle)
        for i, b in enumerate(needle):
            p.needle[i] = b
        return p


class Patterns(C.Structure):
    """kmp_patterns (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("blob", u8p), ("off", u32p), ("len", u32p)]


class Rules(C.Structure):
    """kmp_rules (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("off", u32p), ("terms", u32p)]


KMP_LINK_BUFFER = 64       # KMP_LINK_BUFFER: bytes of a links file's buffer word, the terminator included


class Links(C.Structure):
    """kmp_links (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("buffer", C.POINTER(C.c_char * KMP_LINK_BUFFER)), ("term", u32p)]


class Relation(C.Structure):
    """kmpgpu_relation (include/kmpgpu.h) = kmp_relation (include/kmphost.h)."""
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("dmin", C.c_int32), ("dmax", C.c_int32)]


class Relations(C.Structure):
    """kmp_relations (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("rel", C.POINTER(Relation))]


class ChainLink(C.Structure):
    """kmpgpu_chain_link (include/kmpgpu.h) = kmp_chain_link (include/kmphost.h)."""
    _fields_ = [("pattern", C.c_uint32), ("dmin", C.c_int32), ("dmax", C.c_int32)]


class Chains(C.Structure):
    """kmp_chains (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("off", u32p), ("links", C.POINTER(ChainLink))]


class PktMeta(C.Structure):
    """kmpgpu_pkt_meta (include/kmpgpu.h) = kmp_pkt_meta (include/kmphost.h)."""
    _fields_ = [("src_ip", C.c_uint32), ("dst_ip", C.c_uint32), ("src_port", C.c_uint16), ("dst_port", C.c_uint16),
                ("proto", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class Header(C.Structure):
    """kmpgpu_header (include/kmpgpu.h) = kmp_header (include/kmphost.h)."""
    _fields_ = [("src_ip", C.c_uint32), ("src_mask", C.c_uint32), ("dst_ip", C.c_uint32), ("dst_mask", C.c_uint32),
                ("sport_lo", C.c_uint16), ("sport_hi", C.c_uint16), ("dport_lo", C.c_uint16), ("dport_hi", C.c_uint16),
                ("len_lo", C.c_uint32), ("len_hi", C.c_uint32), ("proto", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint16)]


class Headers(C.Structure):
    """kmp_headers (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("hdr", C.POINTER(Header))]


class ByteTest(C.Structure):
    """kmpgpu_bytetest (include/kmpgpu.h) = kmp_bytetest (include/kmphost.h)."""
    _fields_ = [("anchor", C.c_uint32), ("offset", C.c_int32), ("mask", C.c_uint32), ("value", C.c_uint32),
                ("nbytes", C.c_uint8), ("op", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8)]


class ByteTests(C.Structure):
    """kmp_bytetests (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("bt", C.POINTER(ByteTest))]


class Regexes(C.Structure):
    """kmp_regexes (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("expr", C.POINTER(C.POINTER(C.c_uint8))), ("len", C.POINTER(C.c_uint32)), ("flags", C.POINTER(C.c_uint32)),
                ("gate", C.POINTER(C.c_uint32)), ("bytes", C.POINTER(C.c_uint8)), ("off", C.POINTER(C.c_uint32))]


class Arena(C.Structure):
    """kmp_arena (include/kmphost.h)."""
    _fields_ = [
        ("bytes", u8p), ("nbytes", C.c_uint64), ("off", u64p), ("len", u32p), ("n_pkts", C.c_uint64),
        ("payload_bytes", C.c_uint64), ("n_frames", C.c_uint64), ("free_fn", C.c_void_p),
    ]


class Frames(C.Structure):
    """kmp_frames (include/kmphost.h)."""
    _fields_ = [("bytes", u8p), ("nbytes", C.c_uint64), ("off", u64p), ("caplen", u32p), ("n", C.c_uint64), ("free_fn", C.c_void_p),
                ("map_len", C.c_uint64)]


class Timing(C.Structure):
    """kmpgpu_timing (include/kmpgpu.h)."""
    _fields_ = [("h2d_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double),
                ("launches", C.c_uint32), ("grid_blocks", C.c_uint32), ("h2d_bytes", C.c_uint64)]


class DecodeStats(C.Structure):
    """kmpgpu_decode_stats (include/kmpgpu.h)."""
    _fields_ = [("n_payloads", C.c_uint64), ("n_changed", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64)]


class HttpStats(C.Structure):
    """kmpgpu_http_stats (include/kmpgpu.h)."""
    _fields_ = [("n_requests", C.c_uint64), ("n_responses", C.c_uint64), ("n_blank", C.c_uint64), ("bytes_scanned", C.c_uint64)]


class DnsStats(C.Structure):
    """kmpgpu_dns_stats (include/kmpgpu.h)."""
    _fields_ = [("n_queries", C.c_uint64), ("n_responses", C.c_uint64), ("n_root", C.c_uint64), ("name_bytes", C.c_uint64)]


class DnsSpan(C.Structure):
    """kmpgpu_dns_span (include/kmpgpu.h), 32 bytes."""
    _fields_ = [("kind", C.c_uint8), ("n_labels", C.c_uint8), ("flags", C.c_uint16), ("id", C.c_uint16), ("qtype", C.c_uint16),
                ("qclass", C.c_uint16), ("qdcount", C.c_uint16), ("ancount", C.c_uint16), ("nscount", C.c_uint16), ("arcount", C.c_uint16),
                ("reserved", C.c_uint16), ("name_off", C.c_uint32), ("name_len", C.c_uint32), ("q_end", C.c_uint32)]


class TlsStats(C.Structure):
    """kmpgpu_tls_stats (include/kmpgpu.h)."""
    _fields_ = [("n_hellos", C.c_uint64), ("n_sni", C.c_uint64), ("n_alpn", C.c_uint64), ("n_truncated", C.c_uint64)]


class TlsSpan(C.Structure):
    """kmpgpu_tls_span (include/kmpgpu.h), 32 bytes."""
    _fields_ = [("kind", C.c_uint8), ("flags", C.c_uint8), ("n_ext", C.c_uint8), ("sid_len", C.c_uint8), ("record_version", C.c_uint16),
                ("client_version", C.c_uint16), ("n_suites", C.c_uint16), ("n_alpn", C.c_uint16), ("hs_len", C.c_uint32),
                ("sni_off", C.c_uint32), ("sni_len", C.c_uint32), ("alpn_off", C.c_uint32), ("alpn_len", C.c_uint32)]


class FieldsStats(C.Structure):
    """kmpgpu_fields_stats (include/kmpgpu.h)."""
    _fields_ = [("n_payloads", C.c_uint64), ("n_present", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64)]


class FlowbitOp(C.Structure):
    """kmpgpu_flowbit_op (include/kmpgpu.h)."""
    _fields_ = [("rule", C.c_uint32), ("bit", C.c_uint32), ("op", C.c_uint32), ("reserved", C.c_uint32)]


class Flowbits(C.Structure):
    """kmp_flowbits (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("n_bits", C.c_uint32), ("ops", C.POINTER(FlowbitOp)), ("names", (C.c_char * 32) * 32)]


FLOWBITS_MAX = 32          # KMPGPU_FLOWBITS_MAX
FLOWBIT_OPS = {"isset": 0, "isnotset": 1, "set": 2, "unset": 3, "toggle": 4, "noalert": 5}     # KMPGPU_FB_*


class Threshold(C.Structure):
    """kmpgpu_threshold (include/kmpgpu.h)."""
    _fields_ = [("rule", C.c_uint32), ("track", C.c_uint32), ("type", C.c_uint32), ("count", C.c_uint32), ("window", C.c_uint64)]


class Thresholds(C.Structure):
    """kmp_thresholds (include/kmphost.h)."""
    _fields_ = [("n", C.c_uint32), ("thr", C.POINTER(Threshold))]


THR_TRACKS = {"by_rule": 0, "by_src": 1, "by_dst": 2, "by_flow": 3}           # KMPGPU_THR_BY_*
THR_TYPES = {"at_least": 0, "at_most": 1, "exactly": 2}                       # KMPGPU_THR_AT_LEAST, _AT_MOST, _EXACTLY
THR_NO_WINDOW = 0xFFFFFFFFFFFFFFFF                                            # KMPGPU_THR_NO_WINDOW


class Match(C.Structure):
    """kmpgpu_match (include/kmpgpu.h)."""
    _fields_ = [("packet", C.c_uint64), ("offset", C.c_uint32), ("pattern", C.c_uint32)]


class Alert(C.Structure):
    """kmpgpu_alert (include/kmpgpu.h)."""
    _fields_ = [("packet", C.c_uint64), ("index", C.c_uint32), ("reserved", C.c_uint32)]


# name -> (restype, argtypes); also the list of symbols include/kmphost.h declares
HOST_API = {
    "kmp_pcap_open": (C.c_void_p, [C.c_char_p, C.c_char_p]),
    "kmp_pcap_next": (C.c_int, [C.c_void_p, u32p, u32p, C.POINTER(u8p)]),
    "kmp_pcap_linktype": (C.c_uint32, [C.c_void_p]),
    "kmp_pcap_close": (None, [C.c_void_p]),
    "kmp_extract_udp": (C.c_int, [u8p, C.c_uint32, u32p, u32p]),
    "kmp_extract_tcp": (C.c_int, [u8p, C.c_uint32, u32p, u32p]),
    "kmp_extract_meta": (C.c_int, [u8p, C.c_uint32, C.c_int, C.POINTER(PktMeta)]),
    "kmp_extract_tcp_seq": (C.c_int, [u8p, C.c_uint32, C.c_int, u32p]),
    "kmp_patterns_load": (C.c_int, [C.c_char_p, C.POINTER(Patterns)]),
    "kmp_patterns_parse": (C.c_int, [u8p, C.c_size_t, C.POINTER(Patterns)]),
    "kmp_patterns_free": (None, [C.POINTER(Patterns)]),
    "kmp_rules_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(Rules), C.c_char_p]),
    "kmp_rules_parse_rel": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(Rules), C.c_char_p]),
    "kmp_rules_parse_terms": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Rules), C.c_char_p]),
    "kmp_rules_parse_hdr": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Rules), C.c_char_p]),
    "kmp_rules_free": (None, [C.POINTER(Rules)]),
    "kmp_headers_parse": (C.c_int, [C.c_char_p, C.POINTER(Headers), C.c_char_p]),
    "kmp_headers_free": (None, [C.POINTER(Headers)]),
    "kmp_flowbits_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(Flowbits), C.c_char_p]),
    "kmp_flowbits_free": (None, [C.POINTER(Flowbits)]),
    "kmp_thresholds_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(Thresholds), C.c_char_p]),
    "kmp_thresholds_free": (None, [C.POINTER(Thresholds)]),
    "kmp_rules_parse_bt": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Rules), C.c_char_p]),
    "kmp_bytetests_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(ByteTests), C.c_char_p]),
    "kmp_bytetests_free": (None, [C.POINTER(ByteTests)]),
    "kmp_rules_parse_rx": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Rules), C.c_char_p]),
    "kmp_rules_parse_links": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Rules),
                                        C.c_char_p]),
    "kmp_links_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Links), C.c_char_p]),
    "kmp_links_free": (None, [C.POINTER(Links)]),
    "kmp_regexes_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(Regexes), C.c_char_p]),
    "kmp_regexes_free": (None, [C.POINTER(Regexes)]),
    "kmp_chains_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(Chains), C.c_char_p]),
    "kmp_chains_free": (None, [C.POINTER(Chains)]),
    "kmp_relations_parse": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(Relations), C.c_char_p]),
    "kmp_relations_free": (None, [C.POINTER(Relations)]),
    "kmp_windows_parse": (C.c_int, [C.c_char_p, C.c_uint32, u32p, u32p, C.c_char_p]),
    "kmp_failure_table": (None, [u8p, C.c_uint32, i32p]),
    "kmp_arena_from_pcap": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Arena), C.c_char_p]),
    "kmp_arena_from_pcap_meta": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Arena), C.c_char_p, C.POINTER(C.POINTER(PktMeta))]),
    "kmp_arena_from_pcap_seq": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Arena), C.c_char_p, C.POINTER(C.POINTER(PktMeta)),
                                          C.POINTER(u32p)]),
    "kmp_arena_from_payloads": (C.c_int, [C.POINTER(u8p), u32p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(Arena)]),
    "kmp_arena_layout": (C.c_uint64, [u32p, C.c_uint32, C.c_uint64, C.c_uint32, u64p, u32p]),
    "kmp_arena_free": (None, [C.POINTER(Arena)]),
    "kmp_frames_from_pcap": (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(Frames), C.c_char_p]),
    "kmp_frames_free": (None, [C.POINTER(Frames)]),
    "kmp_batch_open": (C.c_void_p, [C.c_char_p, C.c_int, C.c_char_p]),
    "kmp_batch_next": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, u64p, u64p]),
    "kmp_batch_next_frames": (C.c_int64, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "kmp_batch_file": (C.c_void_p, [C.c_void_p, u64p]),
    "kmp_copy_bytes": (None, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "kmp_batch_close": (None, [C.c_void_p]),
    "kmp_synth_fill_host": (None, [u8p, u64p, u32p, C.c_uint64, C.c_uint64, C.POINTER(SynthParams), C.c_int]),
    "kmp_arena_from_pcap_ts": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Arena), C.c_char_p, C.POINTER(C.POINTER(PktMeta)),
                                         C.POINTER(u64p)]),
    "kmp_arena_from_pcap_seq_ts": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Arena), C.c_char_p, C.POINTER(C.POINTER(PktMeta)),
                                             C.POINTER(u32p), C.POINTER(u64p)]),
    "kmp_synth_count_planted": (C.c_uint64, [u32p, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(SynthParams)]),
    "kmp_report": (None, [C.c_void_p, C.POINTER(Patterns), u64p, C.c_double]),
    "kmp_write_udp_pcap": (C.c_int, [C.c_char_p, u8p, u64p, u32p, C.c_uint64]),
    "kmp_write_udp_pcap_part": (C.c_int, [C.c_char_p, C.c_int, u8p, u64p, u32p, C.c_uint64, C.c_uint64]),
}

# the symbols include/kmpgpu.h declares
GPU_API = {
    "kmpgpu_last_error": (C.c_char_p, []),
    "kmpgpu_device_count": (C.c_int, []),
    "kmpgpu_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "kmpgpu_destroy": (None, [C.c_void_p]),
    "kmpgpu_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kmpgpu_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int64]),
    "kmpgpu_host_alloc": (C.c_void_p, [C.c_size_t]),
    "kmpgpu_host_free": (None, [C.c_void_p]),
    "kmpgpu_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "kmpgpu_host_unregister": (C.c_int, [C.c_void_p]),
    "kmpgpu_set_patterns": (C.c_int, [C.c_void_p, C.POINTER(u8p), u32p, C.c_uint32]),
    "kmpgpu_set_patterns_flags": (C.c_int, [C.c_void_p, C.POINTER(u8p), u32p, u32p, C.c_uint32]),
    "kmpgpu_load_arena": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "kmpgpu_load_frames_begin": (C.c_int, [C.c_void_p, u8p, C.c_uint64, u64p, u32p, C.c_uint64, C.c_int]),
    "kmpgpu_load_frames_finish": (C.c_int, [C.c_void_p, u64p]),
    "kmpgpu_load_frames_uploaded": (C.c_int, [C.c_void_p]),
    "kmpgpu_reserve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
    "kmpgpu_load_frames": (C.c_int, [C.c_void_p, u8p, C.c_uint64, u64p, u32p, C.c_uint64, C.c_int, u64p]),
    "kmpgpu_arena_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p]),
    "kmpgpu_attach_arena": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "kmpgpu_scan": (C.c_int, [C.c_void_p, u64p, C.POINTER(Timing)]),
    "kmpgpu_scan_enqueue": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kmpgpu_counts_device": (C.c_void_p, [C.c_void_p]),
    "kmpgpu_counts_reset": (C.c_int, [C.c_void_p]),
    "kmpgpu_counts_add": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kmpgpu_last_timing": (C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_counts_read": (C.c_int, [C.c_void_p, u64p]),
    "kmpgpu_sync": (C.c_int, [C.c_void_p]),
    "kmpgpu_profile_begin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "kmpgpu_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), u32p]),
    "kmpgpu_scan_offsets": (C.c_int, [C.c_void_p, C.POINTER(Match), C.c_uint64, u64p, u64p]),
    "kmpgpu_scan_packets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_rules": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32]),
    "kmpgpu_scan_rules": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_windows": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32]),
    "kmpgpu_set_relations": (C.c_int, [C.c_void_p, C.POINTER(Relation), C.c_uint32]),
    "kmpgpu_scan_relations": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_chains": (C.c_int, [C.c_void_p, u32p, C.POINTER(ChainLink), C.c_uint32]),
    "kmpgpu_scan_chains": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_meta": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "kmpgpu_meta_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "kmpgpu_set_headers": (C.c_int, [C.c_void_p, C.POINTER(Header), C.c_uint32]),
    "kmpgpu_scan_headers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_bytetests": (C.c_int, [C.c_void_p, C.POINTER(ByteTest), C.c_uint32]),
    "kmpgpu_scan_bytetests": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_regexes": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), u32p, u32p, u32p, C.c_uint32]),
    "kmpgpu_scan_regexes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_links": (C.c_int, [C.c_void_p, C.c_uint32]),
    "kmpgpu_link_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(Timing)]),
    "kmpgpu_scan_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_scan_alerts": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, u64p, u64p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_alerts_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_load_selected": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, u64p]),
    "kmpgpu_load_decoded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(DecodeStats)]),
    "kmpgpu_load_base64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(DecodeStats)]),
    "kmpgpu_http_locate": (C.c_int, [C.c_void_p, C.POINTER(HttpStats)]),
    "kmpgpu_http_spans_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_load_fields": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(FieldsStats)]),
    "kmpgpu_dns_locate": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(DnsStats)]),
    "kmpgpu_dns_spans_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_load_dns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(FieldsStats)]),
    "kmpgpu_tls_locate": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(TlsStats)]),
    "kmpgpu_tls_spans_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_load_tls": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(FieldsStats)]),
    "kmpgpu_flows_build": (C.c_int, [C.c_void_p, C.c_uint32, u64p, C.POINTER(Timing)]),
    "kmpgpu_flows_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_flow_ids_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_scan_flows": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_flowbits": (C.c_int, [C.c_void_p, C.POINTER(FlowbitOp), C.c_uint32, C.c_uint32]),
    "kmpgpu_scan_flowbits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_set_thresholds": (C.c_int, [C.c_void_p, C.POINTER(Threshold), C.c_uint32]),
    "kmpgpu_scan_thresholds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(Timing)]),
    "kmpgpu_flows_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "kmpgpu_load_seams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u64p]),
    "kmpgpu_seams_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_scan_flows_seams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Timing)]),
    "kmpgpu_load_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u64p]),
    "kmpgpu_streams_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_stream_map_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_load_streams_ordered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, u64p]),
    "kmpgpu_stream_segs_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_stream_orders_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "kmpgpu_synth_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SynthParams)]),
    "kmpgpu_fixed_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
    "kmpgpu_arena_info": (C.c_int, [C.c_void_p, u64p, u64p]),
    "kmpgpu_effective_bytes": (C.c_int, [C.c_void_p, u64p]),
    "kmpgpu_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]),
    "kmpgpu_comm_unique_id": (C.c_int, [C.c_void_p]),
    "kmpgpu_comm_init_rank": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "kmpgpu_comm_allreduce_counts": (C.c_int, [C.c_void_p]),
    "kmpgpu_comm_destroy": (None, [C.c_void_p]),
    "kmpgpu_device_of": (C.c_int, [C.c_void_p]),
}


def build(force: bool = False) -> None:
    """Compile libkmpgpu.so (hipcc --offload-arch=gfx950), libkmphost.so and the CLI programs."""
    cmd = ["make", "-s", "-C", CSRC]
    if force:
        subprocess.run(cmd + ["clean"], check=True)
    subprocess.run(cmd, check=True)


def _bind(lib, api):
    for name, (res, args) in api.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_host = None
_gpu = None


def host_lib():
    global _host
    if _host is None:
        if not os.path.isfile(HOST_SO):
            build()
        _host = _bind(C.CDLL(HOST_SO), HOST_API)
    return _host


def gpu_lib():
    """The HIP C-ABI library.  Raises KmpGpuError if it cannot be built or loaded."""
    global _gpu
    if _gpu is None:
        if not os.path.isfile(GPU_SO):
            try:
                build()
            except Exception as e:  # noqa: BLE001
                raise KmpGpuError(f"libkmpgpu.so is missing and could not be built: {e}") from e
        try:
            _gpu = _bind(C.CDLL(GPU_SO), GPU_API)
        except OSError as e:
            raise KmpGpuError(f"cannot load {GPU_SO}: {e}") from e
    return _gpu


def gpu_check(rc: int, what: str) -> None:
    if rc != 0:
        msg = gpu_lib().kmpgpu_last_error()
        raise KmpGpuError(f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
