"""GpuMatcher -- the MI355X hot path behind the C-ABI (include/kmpgpu.h), one context per GPU.

Replaces the reference loop ``string_count[i] += kmp_matcher(payload[k], string[i], prefix[i])``
(serial.c:153-155, openmp_data.c:157-175).  Every method calls straight into libkmpgpu.so; there
is no CPU path here -- a missing library or device raises ``KmpGpuError``.

torch is used for plumbing only (device buffers for the synthetic arena, the current stream,
``torch.distributed`` for the cross-GPU count sum); the C-ABI itself sees raw pointers.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import KmpGpuError, Match, SynthParams, Timing, gpu_check, u8p, u32p, u64p
from .host import BYTETEST_DTYPE, HEADER_DTYPE, META_DTYPE, HostArena

OPT_MODE, OPT_BLOCKS_PER_CU, OPT_DEPTH, OPT_FUSED, OPT_KERNEL, OPT_ACCUMULATE, OPT_NONTEMPORAL = 1, 2, 3, 4, 5, 6, 100
OPT_REPACK = 7
OPT_FUSED_UNIT = 8
OPT_WHOLE_PAYLOAD = 9   # 1: a payload is text up to its end, not up to its first 0x00 (kmpgpu.h, "Semantics")
OPT_KEEP_META = 10      # 1: load_pcap_frames keeps the payloads' header metadata (kmpgpu_pkt_meta) beside the index
OPT_FLOW_SLOTS = 11     # slots of the hash table of build_flows: 0 = auto, or a power of two above the payload count
KERNEL_AUTO, KERNEL_GENERAL, KERNEL_PACKED, KERNEL_FLAT = 0, 1, 2, 3
MODE_FILTER, MODE_AUTOMATON = 0, 1
PAT_NOCASE = 1          # kmpgpu_set_patterns_flags: ASCII letters match either case
ALERT_PATTERNS, ALERT_RULES, ALERT_RELATIONS, ALERT_CHAINS = 0, 1, 2, 3     # KMPGPU_ALERT_*: the row family of scan_alerts
ALERT_FAMILIES = {"patterns": ALERT_PATTERNS, "rules": ALERT_RULES, "relations": ALERT_RELATIONS, "chains": ALERT_CHAINS}
LINK_SAME, LINK_BITMAP, LINK_INDEX, LINK_NONE = 0, 1, 2, 0xFFFFFFFF     # KMPGPU_LINK_*: the map kinds of link_rows
ALERT_DTYPE = np.dtype([("packet", "<u8"), ("index", "<u4"), ("reserved", "<u4")])     # kmpgpu_alert, 16 bytes
ALERTS_ALL = 0xFFFFFFFFFFFFFFFF     # max_records: keep the whole list
FLOW_DIRECTED = 1       # KMPGPU_FLOW_DIRECTED: the two directions of a conversation are two flows
FLOW_SCOPES = {"packet": 0, "flow": 1}     # KMPGPU_FLOW_SCOPE_*
FLOW_DTYPE = np.dtype([("first_packet", "<u8"), ("last_packet", "<u8"), ("n_packets", "<u8"), ("payload_bytes", "<u8"),
                       ("first", META_DTYPE)])     # kmpgpu_flow, 48 bytes
DECODE_PERCENT = 1      # KMPGPU_DECODE_PERCENT: the transform of load_decoded
DECODE_PLUS, DECODE_ONLY_CHANGED = 1, 2     # KMPGPU_DECODE_*: its flags
B64_URLSAFE, B64_ONLY_CHANGED = 1, 2        # KMPGPU_B64_*: the flags of load_base64
FIELD_METHOD, FIELD_RAW_URI, FIELD_STATUS, FIELD_HEADERS, FIELD_BODY = 1, 2, 3, 4, 5       # KMPGPU_FIELD_*: the field of load_fields
FIELDS_ONLY_PRESENT = 1                     # KMPGPU_FIELDS_ONLY_PRESENT: its flag
FIELD_NAMES = {"method": FIELD_METHOD, "raw_uri": FIELD_RAW_URI, "status": FIELD_STATUS, "headers": FIELD_HEADERS, "body": FIELD_BODY}
# kmpgpu_http_span (include/kmpgpu.h)
HTTP_SPAN_DTYPE = np.dtype([("kind", np.uint8), ("flags", np.uint8), ("method_len", np.uint16), ("tok_off", np.uint32), ("tok_len", np.uint32),
                            ("hdr_off", np.uint32), ("hdr_len", np.uint32), ("body_off", np.uint32), ("body_len", np.uint32),
                            ("reserved", np.uint32)])
DNS_QNAME = 1                               # KMPGPU_DNS_QNAME: the field of load_dns
DNS_ONLY_PRESENT, DNS_TCP_PREFIX = 1, 2     # KMPGPU_DNS_*: its flags; DNS_TCP_PREFIX is dns_locate's too
DNS_NONE, DNS_QUERY, DNS_RESPONSE = 0, 1, 2     # kmpgpu_dns_span.kind
DNS_FIELD_NAMES = {"qname": DNS_QNAME}
# kmpgpu_dns_span (include/kmpgpu.h)
DNS_SPAN_DTYPE = np.dtype([("kind", np.uint8), ("n_labels", np.uint8), ("flags", np.uint16), ("id", np.uint16), ("qtype", np.uint16),
                           ("qclass", np.uint16), ("qdcount", np.uint16), ("ancount", np.uint16), ("nscount", np.uint16),
                           ("arcount", np.uint16), ("reserved", np.uint16), ("name_off", np.uint32), ("name_len", np.uint32),
                           ("q_end", np.uint32)])
TLS_SNI, TLS_ALPN = 1, 2                    # KMPGPU_TLS_SNI, KMPGPU_TLS_ALPN: the field of load_tls
TLS_ONLY_PRESENT = 1                        # KMPGPU_TLS_ONLY_PRESENT: its flag
TLS_NONE, TLS_CLIENT_HELLO = 0, 1           # kmpgpu_tls_span.kind
TLS_HAS_SNI, TLS_HAS_ALPN, TLS_TRUNCATED, TLS_ALPN_SKIPPED = 1, 2, 4, 8     # kmpgpu_tls_span.flags
TLS_FIELD_NAMES = {"sni": TLS_SNI, "alpn": TLS_ALPN}
# kmpgpu_tls_span (include/kmpgpu.h)
TLS_SPAN_DTYPE = np.dtype([("kind", np.uint8), ("flags", np.uint8), ("n_ext", np.uint8), ("sid_len", np.uint8), ("record_version", np.uint16),
                           ("client_version", np.uint16), ("n_suites", np.uint16), ("n_alpn", np.uint16), ("hs_len", np.uint32),
                           ("sni_off", np.uint32), ("sni_len", np.uint32), ("alpn_off", np.uint32), ("alpn_len", np.uint32)])
SEAM_DTYPE = np.dtype([("prev", "<u8"), ("next", "<u8"), ("tail_len", "<u4"), ("head_len", "<u4")])      # kmpgpu_seam, 24 bytes
STREAM_DEPTH_MAX = 1 << 30     # KMPGPU_STREAM_DEPTH_MAX
STREAM_DTYPE = np.dtype([("first_packet", "<u8"), ("last_packet", "<u8"), ("n_packets", "<u8"), ("bytes", "<u8"), ("flow", "<u4"),
                         ("dir", "<u4"), ("len", "<u4"), ("reserved", "<u4")])      # kmpgpu_stream, 48 bytes
STREAM_POS_DTYPE = np.dtype([("stream", "<u4"), ("reserved", "<u4"), ("pos", "<u8")])      # kmpgpu_stream_pos, 16 bytes
STREAM_SEG_DTYPE = np.dtype([("skip", "<u4"), ("take", "<u4"), ("seq_off", "<u4"), ("reserved", "<u4")])      # kmpgpu_stream_seg, 16 bytes
STREAM_ORDER_DTYPE = np.dtype([("seq_base", "<u4"), ("n_gaps", "<u4"), ("gap_bytes", "<u8"), ("dup_bytes", "<u8"), ("tcp", "<u4"),
                               ("reserved", "<u4")])      # kmpgpu_stream_order, 32 bytes


def device_count() -> int:
    n = _lib.gpu_lib().kmpgpu_device_count()
    if n < 0:
        gpu_check(n, "kmpgpu_device_count")
    return n


def select_words(select: np.ndarray, n_src: int) -> np.ndarray:
    """The bitmap words kmpgpu_load_selected takes (payload k = bit k & 63 of word k >> 6) from what GpuMatcher.load_selected is
    given on the host: bool[n_src], packed here, or uint64[ceil(n_src / 64)], passed through.  No device needed."""
    W = (n_src + 63) // 64
    select = np.asarray(select)
    if select.dtype == np.bool_:
        if select.shape != (n_src,):
            raise ValueError(f"select: bool{list(select.shape)} for {n_src} payloads")
        b = np.zeros(W * 64, dtype=np.uint8)
        b[:n_src] = select
        return np.packbits(b, bitorder="little").view(np.uint64) if W else np.zeros(0, dtype=np.uint64)
    if select.dtype != np.uint64 or select.shape != (W,):
        raise ValueError(f"select: {select.dtype}{list(select.shape)}; bool[{n_src}] or uint64[{W}] is needed")
    return np.ascontiguousarray(select)


def selected_indices(words: np.ndarray, n_src: int) -> np.ndarray:
    """Ascending indices of the set bits below n_src of uint64 bitmap words: the map from the payloads of a selection back to
    the source's (bits at n_src and above are ignored, as kmpgpu_load_selected ignores them)."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_src]
    return np.flatnonzero(bits).astype(np.uint64)


def stream_locate(stream_map: np.ndarray, stream, offset) -> Tuple[np.ndarray, np.ndarray]:
    """Where the bytes at ``offset`` of the stream payloads ``stream`` come from: (payload, offset_in_payload) in the source of
    load_streams, from its stream_map() (STREAM_POS_DTYPE, one entry per source payload).  Vectorised over equally shaped arrays, so the
    scan_offsets records of a stream context map back to the capture's payloads.  The member is the last one of the stream that starts
    at or before the offset -- of several that start there (empty members in front of it), the one that has the byte.  Offsets are inside
    the stream's len: a byte behind the cut does not occur.  No device needed."""
    stream_map = np.asarray(stream_map)
    if stream_map.dtype != STREAM_POS_DTYPE:
        raise ValueError(f"stream_map: {stream_map.dtype}; STREAM_POS_DTYPE is needed")
    stream = np.asarray(stream, dtype=np.uint64)
    offset = np.asarray(offset, dtype=np.uint64)
    if stream.shape != offset.shape:
        raise ValueError(f"stream{list(stream.shape)} and offset{list(offset.shape)} differ in shape")
    if len(stream_map) == 0:
        if stream.size:
            raise ValueError("stream_locate: stream_map is empty")
        return np.zeros(stream.shape, np.uint64), np.zeros(stream.shape, np.uint64)
    # members in (stream, capture order): pos ascends inside a stream.  Streams are dense (each has a member), so with every stream's
    # positions moved behind those of the stream before it, one ascending key serves one searchsorted for all offsets
    order = np.argsort(stream_map["stream"], kind="stable")
    s_sorted = stream_map["stream"][order].astype(np.int64)
    p_sorted = stream_map["pos"][order]
    n_streams = int(s_sorted[-1]) + 1
    if stream.size and int(stream.max()) >= n_streams:
        raise ValueError(f"stream_locate: stream {int(stream.max())} of {n_streams}")
    last_pos = np.zeros(n_streams, dtype=np.uint64)
    last_pos[s_sorted] = p_sorted                                            # (ascending: the last write is the stream's last member)
    base = np.concatenate(([0], np.cumsum(last_pos + np.uint64(1))[:-1])).astype(np.uint64)
    key = base[s_sorted] + p_sorted
    st = stream.ravel().astype(np.int64)
    j = np.searchsorted(key, base[st] + np.minimum(offset.ravel(), last_pos[st]), side="right") - 1
    return order[j].astype(np.uint64).reshape(stream.shape), (offset.ravel() - p_sorted[j]).reshape(stream.shape)


def stream_locate_ordered(stream_map: np.ndarray, segs: np.ndarray, stream, offset) -> Tuple[np.ndarray, np.ndarray]:
    """stream_locate for streams built with load_streams(seq=...): (payload, offset_in_payload) of the bytes at ``offset`` of the stream
    payloads ``stream``, from stream_map() and stream_segs().  Member k holds the stream's bytes [pos, pos + take), which are its own
    bytes from ``skip`` on; a member of which nothing was kept holds none.  An offset at or behind the stream's last kept byte is a
    ValueError.  No device needed."""
    stream_map, segs = np.asarray(stream_map), np.asarray(segs)
    if stream_map.dtype != STREAM_POS_DTYPE or segs.dtype != STREAM_SEG_DTYPE or stream_map.shape != segs.shape:
        raise ValueError("stream_locate_ordered: STREAM_POS_DTYPE and STREAM_SEG_DTYPE arrays of one length are needed")
    stream = np.asarray(stream, dtype=np.uint64)
    offset = np.asarray(offset, dtype=np.uint64)
    if stream.shape != offset.shape:
        raise ValueError(f"stream{list(stream.shape)} and offset{list(offset.shape)} differ in shape")
    if stream.size == 0:
        return np.zeros(stream.shape, np.uint64), np.zeros(stream.shape, np.uint64)
    kept = np.flatnonzero(segs["take"] > 0)
    # pos < 2^32 * 2^30 and stream < 2^31 do not fit one 64-bit key in general; offsets inside a stream are below 2^31 (the depth), and a
    # member that starts behind that holds no byte anyone asks for
    kept = kept[stream_map["pos"][kept] < np.uint64(1 << 31)]
    key = stream_map["stream"][kept].astype(np.uint64) << np.uint64(31) | stream_map["pos"][kept]
    order = np.argsort(key, kind="stable")
    key, kept = key[order], kept[order]
    if offset.size and int(offset.max()) >= 1 << 31:
        raise ValueError("stream_locate_ordered: an offset of 2^31 or more")
    j = np.searchsorted(key, stream.ravel() << np.uint64(31) | offset.ravel(), side="right") - 1
    k = kept[np.maximum(j, 0)] if kept.size else np.zeros(j.shape, np.int64)
    inside = (j >= 0) & (kept.size > 0)
    if kept.size:
        within = offset.ravel() - stream_map["pos"][k]
        inside &= (stream_map["stream"][k] == stream.ravel()) & (within < segs["take"][k])
    if not inside.all():
        raise ValueError("stream_locate_ordered: an offset behind its stream's last kept byte")
    return k.astype(np.uint64).reshape(stream.shape), (within + segs["skip"][k]).astype(np.uint64).reshape(stream.shape)


class GpuMatcher:
    def __init__(self, device: int = 0, lib=None):
        """lib: another build of libkmpgpu.so, loaded and bound by the caller (tools/windows.py times the parent commit's build next to
        this one); every call of the matcher goes to it.  Default: the package's own library."""
        self._g = lib if lib is not None else _lib.gpu_lib()
        self._ctx = C.c_void_p()
        gpu_check(self._g.kmpgpu_init(C.byref(self._ctx), device), "kmpgpu_init")
        self.device = device
        self.thresholds = []                        # what set_thresholds set: scan_thresholds sizes window_counts by it
        self.patterns: List[bytes] = []
        self.rules: list = []      # (all_of, none_of) per rule, as set_rules took them
        self.windows: list = []    # (first, last) per pattern as set_windows took them (last None: unbounded), [] = none
        self.relations: list = []  # (a, b, dmin, dmax) per relation as set_relations took them (None: unbounded side), [] = none
        self.chains: list = []     # (p0, (p1, dmin, dmax), ...) per chain as set_chains took them (None: unbounded side), [] = none
        self.headers = np.zeros(0, dtype=HEADER_DTYPE)     # the predicates as set_headers took them
        self.bytetests = np.zeros(0, dtype=BYTETEST_DTYPE)  # the byte tests as set_bytetests took them
        self.regexes: list = []    # (expr, flags, gate) per expression as set_regexes took them, [] = none
        self.n_links = 0           # the linked rows set_links reserved
        self._keep = None          # objects whose device memory the context borrows
        self._comm = None          # the GpuComm this matcher is a rank of: closed before the context

    # -- configuration -------------------------------------------------------------------------
    def set_option(self, key: int, value: int) -> None:
        gpu_check(self._g.kmpgpu_set_option(self._ctx, key, value), "kmpgpu_set_option")

    def set_stream(self, hip_stream: Optional[int]) -> None:
        gpu_check(self._g.kmpgpu_set_stream(self._ctx, C.c_void_p(hip_stream or 0)), "kmpgpu_set_stream")

    def set_patterns(self, patterns: Sequence[bytes], nocase=False) -> None:
        """serial.c:148-152: patterns + failure tables (built inside the library).  nocase: a bool for every pattern, or one
        per pattern -- ASCII letters of such a pattern match either case (kmpgpu_set_patterns_flags)."""
        n = len(patterns)
        bufs = [np.frombuffer(p + b"\0", dtype=np.uint8) for p in patterns]
        ptrs = (u8p * max(n, 1))(*[b.ctypes.data_as(u8p) for b in bufs])
        lens = (C.c_uint32 * max(n, 1))(*[len(p) for p in patterns])
        if isinstance(nocase, (bool, int, np.bool_)):
            nocase = [bool(nocase)] * n
        nocase = [bool(x) for x in nocase]
        if len(nocase) != n:
            raise ValueError(f"nocase: {len(nocase)} flags for {n} patterns")
        flags = (C.c_uint32 * max(n, 1))(*[PAT_NOCASE if x else 0 for x in nocase])
        gpu_check(self._g.kmpgpu_set_patterns_flags(self._ctx, ptrs, lens, flags, n), "kmpgpu_set_patterns_flags")
        self.patterns = list(patterns)
        self.rules = []            # the library drops its rules with the pattern set they referred to
        self.windows = []          # ... and its windows
        self.relations = []        # ... and its relations
        self.chains = []           # ... and its chains
        self.headers = np.zeros(0, dtype=HEADER_DTYPE)     # ... and its header predicates
        self.bytetests = np.zeros(0, dtype=BYTETEST_DTYPE)  # ... and its byte tests
        self.regexes = []          # ... and its expressions
        self.n_links = 0           # ... and its links

    def set_rules(self, rules) -> None:
        """Content rules over the current patterns (kmpgpu_set_rules): a sequence of (all_of, none_of) pattern-index sequences;
        a rule matches a payload that holds every pattern of all_of and none of none_of.  An empty sequence clears the rules."""
        rules = [([int(i) for i in a], [int(i) for i in b]) for a, b in rules]
        for a, b in rules:
            for i in a + b:
                if not 0 <= i < _lib.RULE_NOT:
                    raise ValueError(f"rule term {i}: not a pattern index (or rel(q), chain(c), hdr(q), btest(q), regex(q), link(q))")
        off = np.zeros(len(rules) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(a) + len(b) for a, b in rules])
        terms = np.array([t for a, b in rules for t in a + [i | _lib.RULE_NOT for i in b]] or [0], dtype=np.uint32)
        gpu_check(self._g.kmpgpu_set_rules(self._ctx, off.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), len(rules)), "kmpgpu_set_rules")
        self.rules = rules
        self.flowbits, self.n_flowbits = [], 0      # the library drops the flow-bit ops with the rules they referred to
        self.thresholds = []                        # ... and the thresholds

    def set_flowbits(self, ops, n_bits: Optional[int] = None) -> None:
        """Flow-bit tests and actions of the current rules (kmpgpu_set_flowbits): a sequence of (rule, "set" | "unset" | "toggle" |
        "isset" | "isnotset", bit) and (rule, "noalert").  A rule fires for a payload where scan_rules has it AND its tests hold on the
        state of the payload's flow BEFORE that payload; the fired rules' actions, in rule order, make the state the flow's next payload
        sees.  ``n_bits`` None: the highest bit named + 1.  None or an empty sequence clears the ops."""
        rows = []
        for op in (ops or []):
            if len(op) not in (2, 3) or op[1] not in _lib.FLOWBIT_OPS or (len(op) == 2) != (op[1] == "noalert"):
                raise ValueError(f"flow-bit op {op!r}: (rule, {sorted(_lib.FLOWBIT_OPS)}, bit) or (rule, 'noalert') is needed")
            rule, bit = int(op[0]), int(op[2]) if len(op) == 3 else 0
            if not (0 <= rule <= 0xFFFFFFFF and 0 <= bit <= 0xFFFFFFFF):
                raise ValueError(f"flow-bit op {op!r}: rule and bit are 32-bit")
            rows.append((rule, bit, _lib.FLOWBIT_OPS[op[1]]))
        if n_bits is None:
            n_bits = max([b + 1 for _, b, o in rows if o != _lib.FLOWBIT_OPS["noalert"]] or [1])
        arr = (_lib.FlowbitOp * max(len(rows), 1))()
        for a, (rule, bit, op) in zip(arr, rows):
            a.rule, a.bit, a.op, a.reserved = rule, bit, op, 0
        gpu_check(self._g.kmpgpu_set_flowbits(self._ctx, arr if rows else None, len(rows), int(n_bits) if rows else 0), "kmpgpu_set_flowbits")
        self.flowbits, self.n_flowbits = rows, int(n_bits) if rows else 0

    def set_thresholds(self, thresholds) -> None:
        """Rate thresholds of the current rules (kmpgpu_set_thresholds): a sequence of (rule, "by_rule" | "by_src" | "by_dst" | "by_flow",
        "at_least" | "at_most" | "exactly", count, window); window is in the unit of the timestamps scan_thresholds is given, None:
        no window (every earlier payload of the tracker counts).  A rule fires for a payload where scan_rules has it AND, for each of its
        thresholds, the number of its hits in the payload's tracker inside the window -- the payload's own included -- compares as
        asked.  Sliding windows over the rule's hits, not over issued alerts.  None or an empty sequence clears the thresholds."""
        rows = []
        for th in (thresholds or []):
            if len(th) != 5 or th[1] not in _lib.THR_TRACKS or th[2] not in _lib.THR_TYPES:
                raise ValueError(f"threshold {th!r}: (rule, {sorted(_lib.THR_TRACKS)}, {sorted(_lib.THR_TYPES)}, count, window) is needed")
            rule, count, window = int(th[0]), int(th[3]), _lib.THR_NO_WINDOW if th[4] is None else int(th[4])
            if not (0 <= rule <= 0xFFFFFFFF and 0 <= count <= 0xFFFFFFFF and 0 <= window <= _lib.THR_NO_WINDOW):
                raise ValueError(f"threshold {th!r}: rule and count are 32-bit, window is 64-bit")
            rows.append((rule, _lib.THR_TRACKS[th[1]], _lib.THR_TYPES[th[2]], count, window))
        arr = (_lib.Threshold * max(len(rows), 1))()
        for a, (rule, track, typ, count, window) in zip(arr, rows):
            a.rule, a.track, a.type, a.count, a.window = rule, track, typ, count, window
        gpu_check(self._g.kmpgpu_set_thresholds(self._ctx, arr if rows else None, len(rows)), "kmpgpu_set_thresholds")
        self.thresholds = rows

    def set_relations(self, relations) -> None:
        """Distance / within relations between two of the current patterns (kmpgpu_set_relations): a sequence of (a, b, dmin, dmax),
        relation q holding in a payload with an in-window match of a at sa and one of b at sb where dmin <= sb - (sa + len(a)) <= dmax;
        None for dmin or dmax leaves that side unbounded.  None or an empty sequence clears the relations.  Every successful call
        drops the rules, as the library does: set the relations first, then the rules, whose terms may be rel(q)."""
        relations = [(int(a), int(b), None if lo is None else int(lo), None if hi is None else int(hi)) for a, b, lo, hi in (relations or [])]
        for a, b, lo, hi in relations:
            if not (0 <= a <= 0xFFFFFFFF and 0 <= b <= 0xFFFFFFFF):
                raise ValueError(f"relation ({a}, {b}, {lo}, {hi}): pattern indices are 32-bit")
            if not all(x is None or _lib.REL_NO_MIN <= x <= _lib.REL_NO_MAX for x in (lo, hi)):
                raise ValueError(f"relation ({a}, {b}, {lo}, {hi}): bounds are 32-bit")
        arr = (_lib.Relation * max(len(relations), 1))()
        for r, (a, b, lo, hi) in zip(arr, relations):
            r.a, r.b = a, b
            r.dmin = _lib.REL_NO_MIN if lo is None else lo
            r.dmax = _lib.REL_NO_MAX if hi is None else hi
        gpu_check(self._g.kmpgpu_set_relations(self._ctx, arr if relations else None, len(relations)), "kmpgpu_set_relations")
        self.relations = relations
        self.rules = []            # the library drops its rules with the rows they referred to

    def rel(self, q: int) -> int:
        """The term of relation q in set_rules: it is row len(patterns) + q of the hit matrix."""
        if not 0 <= q < len(self.relations):
            raise ValueError(f"rel({q}): {len(self.relations)} relations are set")
        return len(self.patterns) + q

    def set_chains(self, chains) -> None:
        """Content chains over the current patterns (kmpgpu_set_chains): a sequence of (p0, (p1, dmin, dmax), (p2, dmin, dmax), ...), 2 to 8
        contents each; chain c holds in a payload with in-window matches s_0 .. s_{n-1} of p_0 .. p_{n-1} where every content starts
        dmin .. dmax bytes behind the end of THE MATCH of the content before it; None for dmin or dmax leaves that side unbounded.  None
        or an empty sequence clears the chains.  Every successful call drops the rules, as the library does: set the relations, then the
        chains, then the rules, whose terms may be chain(c)."""
        chains = [(int(ch[0]),) + tuple((int(p), None if lo is None else int(lo), None if hi is None else int(hi)) for p, lo, hi in ch[1:])
                  for ch in (chains or [])]
        for ch in chains:
            for p, lo, hi in ((ch[0], None, None),) + ch[1:]:
                if not 0 <= p <= 0xFFFFFFFF:
                    raise ValueError(f"chain {ch}: pattern indices are 32-bit")
                if not all(x is None or _lib.REL_NO_MIN <= x <= _lib.REL_NO_MAX for x in (lo, hi)):
                    raise ValueError(f"chain {ch}: bounds are 32-bit")
        off = np.zeros(len(chains) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(ch) for ch in chains])
        arr = (_lib.ChainLink * max(int(off[-1]), 1))()
        flat = [link for ch in chains for link in ((ch[0], None, None),) + ch[1:]]
        for l, (p, lo, hi) in zip(arr, flat):
            l.pattern = p
            l.dmin = _lib.REL_NO_MIN if lo is None else lo
            l.dmax = _lib.REL_NO_MAX if hi is None else hi
        gpu_check(self._g.kmpgpu_set_chains(self._ctx, off.ctypes.data_as(u32p) if chains else None, arr if chains else None, len(chains)),
                  "kmpgpu_set_chains")
        self.chains = chains
        self.rules = []            # the library drops its rules with the rows they referred to

    def chain(self, c: int) -> int:
        """The term of chain c in set_rules: it is row len(patterns) + len(relations) + c of the hit matrix."""
        if not 0 <= c < len(self.chains):
            raise ValueError(f"chain({c}): {len(self.chains)} chains are set")
        return len(self.patterns) + len(self.relations) + c

    def set_headers(self, headers) -> None:
        """Header predicates (kmpgpu_set_headers): a HEADER_DTYPE array, or a sequence of dicts with any of its fields -- src_ip,
        src_mask, dst_ip, dst_mask, sport_lo, sport_hi, dport_lo, dport_hi, len_lo, len_hi, proto, flags (_lib.HDR_ANY_PROTO,
        _lib.HDR_BIDIR) --, a field left out being "any": mask 0, ports 0..65535, lengths 0..UINT32_MAX; a dict without proto gets
        HDR_ANY_PROTO.  Predicate q holds for a payload by its metadata (set_meta, OPT_KEEP_META) and its length alone.  None or an
        empty sequence clears them.  Every successful call drops the rules, as the library does: relations, chains, headers, then
        the rules, whose terms may be hdr(q)."""
        if isinstance(headers, np.ndarray) and headers.dtype == HEADER_DTYPE:
            arr = np.ascontiguousarray(headers)
        else:
            arr = np.zeros(len(headers or []), dtype=HEADER_DTYPE)
            for r, h in zip(arr, headers or []):
                r["sport_hi"] = r["dport_hi"] = 0xFFFF
                r["len_hi"] = 0xFFFFFFFF
                if "proto" not in h:
                    r["flags"] = _lib.HDR_ANY_PROTO
                for k, v in h.items():
                    r[k] = (int(r[k]) | int(v)) if k == "flags" else int(v)
        gpu_check(self._g.kmpgpu_set_headers(self._ctx, C.cast(arr.ctypes.data, C.POINTER(_lib.Header)) if arr.size else None, int(arr.size)),
                  "kmpgpu_set_headers")
        self.headers = arr.copy()
        self.rules = []            # the library drops its rules with the rows they referred to

    def hdr(self, q: int) -> int:
        """The term of header predicate q in set_rules: it is row len(patterns) + len(relations) + len(chains) + q of the hit matrix."""
        if not 0 <= q < len(self.headers):
            raise ValueError(f"hdr({q}): {len(self.headers)} header predicates are set")
        return len(self.patterns) + len(self.relations) + len(self.chains) + q

    def set_bytetests(self, tests) -> None:
        """Byte tests (kmpgpu_set_bytetests): a BYTETEST_DTYPE array, or a sequence of dicts with nbytes (1..4), op (_lib.BT_EQ .. BT_GE),
        value and offset, and any of mask (left out: all bits), anchor (a pattern index: the test is relative, its offset counts from the
        end of a match of that pattern; _lib.BT_RELATIVE is set for it) and flags (_lib.BT_LITTLE; default big-endian).  Test q holds for
        a payload where ((field & mask) op value) for the unsigned integer the nbytes bytes at the position form, all of them in front
        of the payload's text end.  None or an empty sequence clears them.  Every successful call drops the rules, as the library does:
        relations, chains, headers, byte tests, then the rules, whose terms may be btest(q)."""
        if isinstance(tests, np.ndarray) and tests.dtype == BYTETEST_DTYPE:
            arr = np.ascontiguousarray(tests)
        else:
            arr = np.zeros(len(tests or []), dtype=BYTETEST_DTYPE)
            for r, b in zip(arr, tests or []):
                r["mask"] = 0xFFFFFFFF
                if "anchor" in b:
                    r["flags"] = _lib.BT_RELATIVE
                for k, v in b.items():
                    r[k] = (int(r[k]) | int(v)) if k == "flags" else int(v)
        gpu_check(self._g.kmpgpu_set_bytetests(self._ctx, C.cast(arr.ctypes.data, C.POINTER(_lib.ByteTest)) if arr.size else None, int(arr.size)),
                  "kmpgpu_set_bytetests")
        self.bytetests = arr.copy()
        self.rules = []            # the library drops its rules with the rows they referred to

    def btest(self, q: int) -> int:
        """The term of byte test q in set_rules: it is row len(patterns) + len(relations) + len(chains) + len(headers) + q of the hit matrix."""
        if not 0 <= q < len(self.bytetests):
            raise ValueError(f"btest({q}): {len(self.bytetests)} byte tests are set")
        return len(self.patterns) + len(self.relations) + len(self.chains) + len(self.headers) + q

    def set_regexes(self, exprs) -> None:
        """Expressions of byte classes and repeats (kmpgpu_set_regexes; the dialect is in include/kmpgpu.h): a sequence whose entries are
        ``bytes``, or ``(bytes, dict)`` with any of nocase (ASCII case-insensitive), dotall (. matches 0x0A too), groups (( ) (?: ) and | are part of the dialect) and gate (a pattern index:
        the expression is looked at only in payloads that hold that pattern).  Expression q hits a payload where some part of its text,
        up to the text end, is in the expression's language (^: from the first byte, $: up to the text end).  None or an empty sequence
        clears them.  Every successful call drops the rules, as the library does: relations, chains, headers, byte tests, regexes, then
        the rules, whose terms may be regex(q)."""
        took = []
        for e in exprs or []:
            expr, opt = (e, {}) if isinstance(e, (bytes, bytearray)) else e
            unknown = set(opt) - {"nocase", "dotall", "gate", "groups"}
            if unknown:
                raise ValueError(f"set_regexes: unknown option(s) {sorted(unknown)}")
            gate = opt.get("gate")
            flags = ((_lib.RX_NOCASE if opt.get("nocase") else 0) | (_lib.RX_DOTALL if opt.get("dotall") else 0)
                     | (0 if gate is None else _lib.RX_GATED) | (_lib.RX_GROUPS if opt.get("groups") else 0))
            took.append((bytes(expr), flags, 0 if gate is None else int(gate)))
        n = len(took)
        bufs = [C.create_string_buffer(e, len(e)) for e, _, _ in took]      # (an expression may hold any byte, escaped or not)
        ptrs = (C.c_char_p * max(n, 1))(*[C.cast(b, C.c_char_p) for b in bufs])
        lens = np.array([len(e) for e, _, _ in took] or [0], dtype=np.uint32)
        flags = np.array([f for _, f, _ in took] or [0], dtype=np.uint32)
        gates = np.array([g for _, _, g in took] or [0], dtype=np.uint32)
        gpu_check(self._g.kmpgpu_set_regexes(self._ctx, ptrs if n else None, lens.ctypes.data_as(u32p) if n else None,
                                             flags.ctypes.data_as(u32p), gates.ctypes.data_as(u32p), n), "kmpgpu_set_regexes")
        self.regexes = took
        self.rules = []            # the library drops its rules with the rows they referred to

    def regex(self, q: int) -> int:
        """The term of expression q in set_rules: it is row len(patterns) + len(relations) + len(chains) + len(headers) + len(bytetests) + q
        of the hit matrix."""
        if not 0 <= q < len(self.regexes):
            raise ValueError(f"regex({q}): {len(self.regexes)} expressions are set")
        return len(self.patterns) + len(self.relations) + len(self.chains) + len(self.headers) + len(self.bytetests) + q

    def set_links(self, n: int) -> None:
        """Reserve ``n`` linked rows behind the expressions' rows (kmpgpu_set_links): rows another matcher computes over its own view of
        these payloads, filled by link_rows() and named in set_rules as link(q).  0 clears them.  Every successful call drops the rules,
        as the library does, and leaves every link unfilled."""
        gpu_check(self._g.kmpgpu_set_links(self._ctx, int(n)), "kmpgpu_set_links")
        self.n_links = int(n)
        self.rules = []            # the library drops its rules with the rows they referred to

    def link(self, q: int) -> int:
        """The term of link q in set_rules: it is row len(patterns) + len(relations) + len(chains) + len(headers) + len(bytetests) +
        len(regexes) + q of the hit matrix."""
        if not 0 <= q < self.n_links:
            raise ValueError(f"link({q}): {self.n_links} links are set")
        return len(self.patterns) + len(self.relations) + len(self.chains) + len(self.headers) + len(self.bytetests) + len(self.regexes) + q

    def link_rows(self, first_link: int, src: "GpuMatcher", family: str = "rules", rows=None, map=None) -> Timing:
        """Fill links first_link, first_link + 1, ... of this matcher from rows of ``src``'s family ("patterns", "rules", "relations",
        "chains"), translated on the device into this matcher's payload numbering (kmpgpu_link_rows; src's pass for the family runs
        inside).  rows: None for all rows of the family, a range of consecutive rows, or one row.  map says which payload of src payload k
        of this matcher is: None -- the same k (the payload counts must be equal); a bool[n] array or uint64 words -- the j-th set bit
        is src's payload j (the ``changed`` / ``present`` of the derived-arena loaders, the select of load_selected); a uint32[n] array
        -- src's payload for each of this matcher's, a value >= src's payload count (LINK_NONE) for none (stream_map()["stream"]); or a
        contiguous torch tensor on the device, of 64-bit words for the bitmap and 32-bit values for the index.  Returns the timing of
        the translation."""
        fam = ALERT_FAMILIES
        if family not in fam:
            raise ValueError(f"link_rows: family {family!r}; one of {sorted(fam)} is needed")
        n_fam = {"patterns": len(src.patterns), "rules": len(src.rules), "relations": len(src.relations), "chains": len(src.chains)}[family]
        if rows is None:
            first_row, n_rows = 0, n_fam
        elif isinstance(rows, range):
            if rows.step != 1:
                raise ValueError("link_rows: rows must be consecutive")
            first_row, n_rows = rows.start, len(rows)
        else:
            first_row, n_rows = int(rows), 1
        n_dst, _ = self.arena_info()
        W = (n_dst + 63) // 64
        kind, ptr, on_device, keep = LINK_SAME, None, 0, None
        if map is None:
            pass
        elif isinstance(map, np.ndarray):
            if map.dtype == np.uint32:
                if map.shape != (n_dst,):
                    raise ValueError(f"map: uint32{list(map.shape)} for {n_dst} payloads")
                kind, keep = LINK_INDEX, np.ascontiguousarray(map)
            else:
                kind, keep = LINK_BITMAP, select_words(map, n_dst)
            ptr = keep.ctypes.data if n_dst else None
        else:                                     # a torch tensor on the device
            if not map.is_cuda or map.device.index != self.device or not map.is_contiguous() or map.dtype.is_floating_point \
                    or map.dtype.itemsize not in (4, 8) or map.numel() != (W if map.dtype.itemsize == 8 else n_dst):
                raise ValueError(f"map: a contiguous tensor of {W} 64-bit words or {n_dst} 32-bit values on the matcher's device is needed")
            import torch
            torch.cuda.current_stream(map.device).synchronize()              # complete before the call (kmpgpu.h)
            kind = LINK_BITMAP if map.dtype.itemsize == 8 else LINK_INDEX
            ptr, on_device, keep = (map.data_ptr() if n_dst else None), 1, map
        t = Timing()
        gpu_check(self._g.kmpgpu_link_rows(self._ctx, int(first_link), src._ctx, fam[family], first_row, n_rows, kind, ptr, on_device,
                                           C.byref(t)), "kmpgpu_link_rows")
        del keep
        return t

    def scan_links(self, hits: bool = False) -> dict:
        """The linked rows as this matcher holds them (kmpgpu_scan_links): the marking pass of scan_packets and the copy of the link
        buffer; an unfilled link reads as no payload.  A dict as scan_packets returns, with ``link_pkt_counts`` (uint64[n_links])."""
        return self._scan_family("kmpgpu_scan_links", self.n_links, "link_pkt_counts", hits)

    def set_meta(self, meta) -> None:
        """The per-payload header metadata of the arena at hand (kmpgpu_set_meta): a META_DTYPE array with one record per payload
        (HostArena.from_pcap(..., with_meta=True).meta), or a contiguous torch tensor of 16 bytes per payload on this matcher's
        device, copied on the device.  None clears the metadata."""
        if meta is None:
            gpu_check(self._g.kmpgpu_set_meta(self._ctx, None, 0, 0), "kmpgpu_set_meta")
        elif isinstance(meta, np.ndarray):
            if meta.dtype != META_DTYPE:
                raise ValueError(f"meta: {meta.dtype}; META_DTYPE is needed")
            m = np.ascontiguousarray(meta)
            gpu_check(self._g.kmpgpu_set_meta(self._ctx, m.ctypes.data if m.size else None, int(m.size), 0), "kmpgpu_set_meta")
        else:                                     # a torch tensor
            nbytes = meta.numel() * meta.element_size()
            if not meta.is_cuda or meta.device.index != self.device or not meta.is_contiguous() or nbytes % 16:
                raise ValueError("meta: a contiguous tensor of 16 bytes per payload on the matcher's device is needed")
            import torch
            torch.cuda.current_stream(meta.device).synchronize()
            gpu_check(self._g.kmpgpu_set_meta(self._ctx, meta.data_ptr() if nbytes else None, nbytes // 16, 1), "kmpgpu_set_meta")

    def meta(self) -> np.ndarray:
        """The metadata the context holds, META_DTYPE[n_pkts] (kmpgpu_meta_download); KmpGpuError where it has none."""
        n = C.c_uint64()
        gpu_check(self._g.kmpgpu_meta_download(self._ctx, None, 0, C.byref(n)), "kmpgpu_meta_download")
        out = np.zeros(max(int(n.value), 1), dtype=META_DTYPE)
        gpu_check(self._g.kmpgpu_meta_download(self._ctx, out.ctypes.data, out.size, C.byref(n)), "kmpgpu_meta_download")
        return out[: int(n.value)]

    def set_windows(self, windows) -> None:
        """Offset windows of the current patterns (kmpgpu_set_windows): one (first, last) per pattern, last None = unbounded;
        scan_offsets, scan_packets and scan_rules then report, mark and combine only the matches that start at first..last of
        their payload.  scan() and every counts output are not affected.  None or an empty sequence clears the windows."""
        windows = [(int(a), None if b is None else int(b)) for a, b in (windows or [])]
        if not windows:
            gpu_check(self._g.kmpgpu_set_windows(self._ctx, None, None, 0), "kmpgpu_set_windows")
            self.windows = []
            return
        for a, b in windows:
            if not 0 <= a <= 0xFFFFFFFF or not (b is None or 0 <= b <= 0xFFFFFFFF):
                raise ValueError(f"window ({a}, {b}): offsets are 32-bit")
        first = np.array([a for a, _ in windows], dtype=np.uint32)
        last = np.array([0xFFFFFFFF if b is None else b for _, b in windows], dtype=np.uint32)
        gpu_check(self._g.kmpgpu_set_windows(self._ctx, first.ctypes.data_as(u32p), last.ctypes.data_as(u32p), len(windows)), "kmpgpu_set_windows")
        self.windows = windows

    # -- arena ------------------------------------------------------------------------------------
    def load_arena(self, arena, off: Optional[np.ndarray] = None, ln: Optional[np.ndarray] = None) -> None:
        """Upload a host arena (HostArena, or numpy bytes + off + len)."""
        meta = None
        if isinstance(arena, HostArena):
            a, off, ln, meta = arena.bytes, arena.off, arena.len, arena.meta
        else:
            a = np.ascontiguousarray(arena, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        n = int(ln.shape[0])
        gpu_check(self._g.kmpgpu_load_arena(self._ctx, a.ctypes.data if a.size else None, int(a.size),
                                            off.ctypes.data if n else None, ln.ctypes.data if n else None, n),
                  "kmpgpu_load_arena")
        self._keep = None
        if meta is not None and n:                # an arena built with_meta brings its metadata along
            self.set_meta(meta)

    def attach_arena(self, d_arena, d_off, d_len, arena_bytes: Optional[int] = None) -> None:
        """Borrow a device-resident arena: torch uint8 / int64 / int32 CUDA tensors.  arena_bytes: what the library is
        told the arena holds (default: the whole tensor); the end of the last slot is enough."""
        n = int(d_len.numel())
        nb = int(d_arena.numel()) if arena_bytes is None else int(arena_bytes)
        gpu_check(self._g.kmpgpu_attach_arena(self._ctx, d_arena.data_ptr(), nb, d_off.data_ptr(),
                                              d_len.data_ptr(), n), "kmpgpu_attach_arena")
        self._keep = (d_arena, d_off, d_len)

    def load_pcap_frames(self, path: str, proto: str = "udp", rank: int = 0, world: int = 1) -> Tuple[int, int]:
        """Upload the raw capture and extract the payloads on the GPU (kmpgpu_load_frames).  With world > 1
        only this rank's share of the FRAMES is extracted (n / world each, the remainder to rank 0:
        mpi_dumping.c:149-157).  Returns (payloads accepted, frames in the file)."""
        from .dist import shard_range
        H = _lib.host_lib()
        fr = _lib.Frames()
        err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
        rc = H.kmp_frames_from_pcap(path.encode(), None, None, C.byref(fr), err)
        if rc:
            raise _lib.KmpHostError(f"error reading pcap file: {err.value.decode(errors='replace')} ({rc})")
        try:
            n = C.c_uint64()
            lo, hi = shard_range(int(fr.n), rank, world)
            off = C.cast(C.addressof(fr.off.contents) + 8 * lo, _lib.u64p) if fr.n else fr.off
            cl = C.cast(C.addressof(fr.caplen.contents) + 4 * lo, _lib.u32p) if fr.n else fr.caplen
            gpu_check(self._g.kmpgpu_load_frames(self._ctx, fr.bytes, fr.nbytes, off, cl, hi - lo, 1 if proto == "tcp" else 0,
                                                 C.byref(n)), "kmpgpu_load_frames")
            self._keep = None
            return int(n.value), int(fr.n)
        finally:
            H.kmp_frames_free(C.byref(fr))

    def load_selected(self, src: "GpuMatcher", select) -> np.ndarray:
        """Make this matcher's arena the payloads of ``src`` that ``select`` picks, compacted on the device in ascending source
        order (kmpgpu_load_selected); patterns, rules, windows and options of this matcher stay.  select: a bool[n_src] numpy
        array (packed here), a uint64[W] numpy array of bitmap words as scan_packets lays them out (W = ceil(n_src / 64)), or
        a torch tensor of W 64-bit words (int64 / uint64) on src's device, which is handed over as it is.  Returns the source
        indices of the selected payloads: payload j of this matcher is payload result[j] of src (for a device bitmap the words
        are copied to the host once for this)."""
        n_src, _ = src.arena_info()
        W = (n_src + 63) // 64
        on_device = 0
        if isinstance(select, np.ndarray):
            words = select_words(select, n_src)
            ptr = words.ctypes.data if W else None
        else:                                     # a torch tensor
            if select.dtype.itemsize != 8 or select.dtype.is_floating_point or select.numel() != W:
                raise ValueError(f"select: a tensor of {W} 64-bit words is needed for {n_src} payloads")
            if select.is_cuda:
                if select.device.index != src.device or not select.is_contiguous():
                    raise ValueError("select: the tensor must be contiguous and on the source's device")
                import torch
                torch.cuda.current_stream(select.device).synchronize()       # complete before the call (kmpgpu.h)
                on_device, ptr = 1, (select.data_ptr() if W else None)
                words = select.cpu().numpy().view(np.uint64).reshape(-1)
            else:
                words = np.ascontiguousarray(select.numpy()).view(np.uint64).reshape(-1)
                ptr = words.ctypes.data if W else None
        n = C.c_uint64()
        gpu_check(self._g.kmpgpu_load_selected(self._ctx, src._ctx, ptr, on_device, C.byref(n)), "kmpgpu_load_selected")
        self._keep = None
        idx = selected_indices(words, n_src)
        if idx.size != int(n.value):
            raise KmpGpuError(f"kmpgpu_load_selected reports {int(n.value)} payloads, the bitmap holds {idx.size}")
        return idx

    def load_decoded(self, src: "GpuMatcher", plus: bool = False, only_changed: bool = False) -> dict:
        """Make this matcher's arena the payloads of ``src`` percent-decoded on the device (kmpgpu_load_decoded; the definition:
        kmpgpu.h -- what urllib.parse.unquote_to_bytes computes, with ``plus`` after '+' was replaced by ' '); patterns, rules,
        windows and options of this matcher stay.  only_changed: this matcher holds only the payloads the decoding changes,
        compacted in ascending source order.  Returns {"changed": bool[n_src], "index": int64[n_dst], "stats": {...}}: payload j
        of this matcher is the decoding of payload index[j] of src."""
        flags = (DECODE_PLUS if plus else 0) | (DECODE_ONLY_CHANGED if only_changed else 0)
        return self._load_recoded(src, "kmpgpu_load_decoded", only_changed,
                                  lambda words, st: self._g.kmpgpu_load_decoded(self._ctx, src._ctx, DECODE_PERCENT, flags, words, None, st))

    def load_base64(self, src: "GpuMatcher", min_run: int = 16, urlsafe: bool = False, only_changed: bool = False) -> dict:
        """Make this matcher's arena the payloads of ``src`` with their base64 runs of ``min_run`` (4..255) alphabet bytes and more
        decoded on the device (kmpgpu_load_base64; the definition: kmpgpu.h -- base64.b64decode run by run, urlsafe_b64decode with
        ``urlsafe``); patterns, rules, windows and options of this matcher stay.  only_changed: this matcher holds only the payloads
        with a decoded run, compacted in ascending source order.  Returns what load_decoded returns."""
        flags = (B64_URLSAFE if urlsafe else 0) | (B64_ONLY_CHANGED if only_changed else 0)
        return self._load_recoded(src, "kmpgpu_load_base64", only_changed,
                                  lambda words, st: self._g.kmpgpu_load_base64(self._ctx, src._ctx, int(min_run), flags, words, None, st))

    def _load_recoded(self, src: "GpuMatcher", what: str, only_changed: bool, call) -> dict:
        n_src, _ = src.arena_info()
        W = (n_src + 63) // 64
        words = np.zeros(max(W, 1), dtype=np.uint64)
        st = _lib.DecodeStats()
        gpu_check(call(words.ctypes.data, C.byref(st)), what)
        self._keep = None
        bits = np.unpackbits(words[:W].view(np.uint8), bitorder="little")
        if bits[n_src:].any():
            raise KmpGpuError(f"{what} set a bit at or above {n_src} in the changed bitmap")
        changed = bits[:n_src].astype(bool)
        index = np.flatnonzero(changed).astype(np.int64) if only_changed else np.arange(n_src, dtype=np.int64)
        stats = {f: int(getattr(st, f)) for f, _ in _lib.DecodeStats._fields_}
        if stats["n_changed"] != int(changed.sum()) or stats["n_payloads"] != index.size or self.arena_info()[0] != index.size:
            raise KmpGpuError(f"{what} reports {stats['n_payloads']} payloads and {stats['n_changed']} changed ones, the "
                              f"bitmap holds {int(changed.sum())} of {n_src}")
        return {"changed": changed, "index": index, "stats": stats}

    def http_locate(self) -> dict:
        """Locate the HTTP message at the start of every payload of this matcher's arena (kmpgpu_http_locate; the definition:
        kmpgpu.h).  The spans stay on the device until the arena changes; with valid spans nothing is launched.  Returns the
        stats: {"n_requests", "n_responses", "n_blank", "bytes_scanned"}."""
        st = _lib.HttpStats()
        gpu_check(self._g.kmpgpu_http_locate(self._ctx, C.byref(st)), "kmpgpu_http_locate")
        return {f: int(getattr(st, f)) for f, _ in _lib.HttpStats._fields_}

    def http_spans(self) -> np.ndarray:
        """The kmpgpu_http_span records of the last http_locate() / load_fields() over this matcher's arena, one per payload, as
        a structured array (HTTP_SPAN_DTYPE)."""
        n, _ = self.arena_info()
        out = np.zeros(max(n, 1), dtype=HTTP_SPAN_DTYPE)
        gpu_check(self._g.kmpgpu_http_spans_read(self._ctx, out.ctypes.data, 0, n), "kmpgpu_http_spans_read")
        return out[:n]

    def load_fields(self, src: "GpuMatcher", field: str = "raw_uri", only_present: bool = False) -> dict:
        """Make this matcher's arena one HTTP field of every payload of ``src`` (kmpgpu_load_fields; the definition: kmpgpu.h);
        patterns, rules, windows and options of this matcher stay.  field: "method", "raw_uri", "status", "headers" or "body".
        only_present: this matcher holds only the payloads that have the field, compacted in ascending source order.  Returns
        {"present": bool[n_src], "index": int64[n_dst], "stats": {...}}: payload j of this matcher is the field of payload
        index[j] of src."""
        if field not in FIELD_NAMES:
            raise ValueError(f"field: {field!r} is none of {', '.join(FIELD_NAMES)}")
        n_src, _ = src.arena_info()
        W = (n_src + 63) // 64
        words = np.zeros(max(W, 1), dtype=np.uint64)
        st = _lib.FieldsStats()
        flags = FIELDS_ONLY_PRESENT if only_present else 0
        gpu_check(self._g.kmpgpu_load_fields(self._ctx, src._ctx, FIELD_NAMES[field], flags, words.ctypes.data, None, C.byref(st)),
                  "kmpgpu_load_fields")
        self._keep = None
        bits = np.unpackbits(words[:W].view(np.uint8), bitorder="little")
        if bits[n_src:].any():
            raise KmpGpuError(f"kmpgpu_load_fields set a bit at or above {n_src} in the present bitmap")
        present = bits[:n_src].astype(bool)
        index = np.flatnonzero(present).astype(np.int64) if only_present else np.arange(n_src, dtype=np.int64)
        stats = {f: int(getattr(st, f)) for f, _ in _lib.FieldsStats._fields_}
        if stats["n_present"] != int(present.sum()) or stats["n_payloads"] != index.size or self.arena_info()[0] != index.size:
            raise KmpGpuError(f"kmpgpu_load_fields reports {stats['n_payloads']} payloads and {stats['n_present']} present ones, the "
                              f"bitmap holds {int(present.sum())} of {n_src}")
        return {"present": present, "index": index, "stats": stats}

    def dns_locate(self, tcp_prefix: bool = False) -> dict:
        """Locate the first question of the DNS message in every payload of this matcher's arena (kmpgpu_dns_locate; the definition:
        kmpgpu.h).  tcp_prefix: a 2-byte length stands in front of every message.  The spans stay on the device until the arena
        changes; with valid spans of the same tcp_prefix nothing is launched.  Returns the stats: {"n_queries", "n_responses",
        "n_root", "name_bytes"}."""
        st = _lib.DnsStats()
        gpu_check(self._g.kmpgpu_dns_locate(self._ctx, DNS_TCP_PREFIX if tcp_prefix else 0, C.byref(st)), "kmpgpu_dns_locate")
        return {f: int(getattr(st, f)) for f, _ in _lib.DnsStats._fields_}

    def dns_spans(self) -> np.ndarray:
        """The kmpgpu_dns_span records of the last dns_locate() / load_dns() over this matcher's arena, one per payload, as a
        structured array (DNS_SPAN_DTYPE)."""
        n, _ = self.arena_info()
        out = np.zeros(max(n, 1), dtype=DNS_SPAN_DTYPE)
        gpu_check(self._g.kmpgpu_dns_spans_read(self._ctx, out.ctypes.data, 0, n), "kmpgpu_dns_spans_read")
        return out[:n]

    def load_dns(self, src: "GpuMatcher", field: str = "qname", only_present: bool = False, tcp_prefix: bool = False) -> dict:
        """Make this matcher's arena the dotted name of the first DNS question of every payload of ``src`` (kmpgpu_load_dns; the
        definition: kmpgpu.h); patterns, rules, windows and options of this matcher stay.  only_present: this matcher holds only
        the payloads that are DNS messages, compacted in ascending source order.  Returns what load_fields returns:
        {"present": bool[n_src], "index": int64[n_dst], "stats": {...}}."""
        if field not in DNS_FIELD_NAMES:
            raise ValueError(f"field: {field!r} is none of {', '.join(DNS_FIELD_NAMES)}")
        n_src, _ = src.arena_info()
        W = (n_src + 63) // 64
        words = np.zeros(max(W, 1), dtype=np.uint64)
        st = _lib.FieldsStats()
        flags = (DNS_ONLY_PRESENT if only_present else 0) | (DNS_TCP_PREFIX if tcp_prefix else 0)
        gpu_check(self._g.kmpgpu_load_dns(self._ctx, src._ctx, DNS_FIELD_NAMES[field], flags, words.ctypes.data, None, C.byref(st)),
                  "kmpgpu_load_dns")
        self._keep = None
        bits = np.unpackbits(words[:W].view(np.uint8), bitorder="little")
        if bits[n_src:].any():
            raise KmpGpuError(f"kmpgpu_load_dns set a bit at or above {n_src} in the present bitmap")
        present = bits[:n_src].astype(bool)
        index = np.flatnonzero(present).astype(np.int64) if only_present else np.arange(n_src, dtype=np.int64)
        stats = {f: int(getattr(st, f)) for f, _ in _lib.FieldsStats._fields_}
        if stats["n_present"] != int(present.sum()) or stats["n_payloads"] != index.size or self.arena_info()[0] != index.size:
            raise KmpGpuError(f"kmpgpu_load_dns reports {stats['n_payloads']} payloads and {stats['n_present']} present ones, the "
                              f"bitmap holds {int(present.sum())} of {n_src}")
        return {"present": present, "index": index, "stats": stats}

    def tls_locate(self) -> dict:
        """Locate the server name and the ALPN list of the TLS ClientHello in every payload of this matcher's arena (kmpgpu_tls_locate;
        the definition: kmpgpu.h).  The spans stay on the device until the arena changes; with valid spans nothing is launched.
        Returns the stats: {"n_hellos", "n_sni", "n_alpn", "n_truncated"}."""
        st = _lib.TlsStats()
        gpu_check(self._g.kmpgpu_tls_locate(self._ctx, 0, C.byref(st)), "kmpgpu_tls_locate")
        return {f: int(getattr(st, f)) for f, _ in _lib.TlsStats._fields_}

    def tls_spans(self) -> np.ndarray:
        """The kmpgpu_tls_span records of the last tls_locate() / load_tls() over this matcher's arena, one per payload, as a
        structured array (TLS_SPAN_DTYPE)."""
        n, _ = self.arena_info()
        out = np.zeros(max(n, 1), dtype=TLS_SPAN_DTYPE)
        gpu_check(self._g.kmpgpu_tls_spans_read(self._ctx, out.ctypes.data, 0, n), "kmpgpu_tls_spans_read")
        return out[:n]

    def load_tls(self, src: "GpuMatcher", field: str = "sni", only_present: bool = False) -> dict:
        """Make this matcher's arena the server name ("sni") or the ALPN list as ``h2,http/1.1`` ("alpn") of the ClientHello in every
        payload of ``src`` (kmpgpu_load_tls; the definition: kmpgpu.h); patterns, rules, windows and options of this matcher stay.
        only_present: this matcher holds only the payloads that have the field, compacted in ascending source order.  Returns what
        load_fields returns: {"present": bool[n_src], "index": int64[n_dst], "stats": {...}}."""
        if field not in TLS_FIELD_NAMES:
            raise ValueError(f"field: {field!r} is none of {', '.join(TLS_FIELD_NAMES)}")
        n_src, _ = src.arena_info()
        W = (n_src + 63) // 64
        words = np.zeros(max(W, 1), dtype=np.uint64)
        st = _lib.FieldsStats()
        gpu_check(self._g.kmpgpu_load_tls(self._ctx, src._ctx, TLS_FIELD_NAMES[field], TLS_ONLY_PRESENT if only_present else 0,
                                          words.ctypes.data, None, C.byref(st)), "kmpgpu_load_tls")
        self._keep = None
        bits = np.unpackbits(words[:W].view(np.uint8), bitorder="little")
        if bits[n_src:].any():
            raise KmpGpuError(f"kmpgpu_load_tls set a bit at or above {n_src} in the present bitmap")
        present = bits[:n_src].astype(bool)
        index = np.flatnonzero(present).astype(np.int64) if only_present else np.arange(n_src, dtype=np.int64)
        stats = {f: int(getattr(st, f)) for f, _ in _lib.FieldsStats._fields_}
        if stats["n_present"] != int(present.sum()) or stats["n_payloads"] != index.size or self.arena_info()[0] != index.size:
            raise KmpGpuError(f"kmpgpu_load_tls reports {stats['n_payloads']} payloads and {stats['n_present']} present ones, the "
                              f"bitmap holds {int(present.sum())} of {n_src}")
        return {"present": present, "index": index, "stats": stats}

    def arena_download(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        n, _ = self.arena_info()
        nb = C.c_uint64()
        gpu_check(self._g.kmpgpu_arena_download(self._ctx, None, 0, C.byref(nb), None, None), "kmpgpu_arena_download")
        a = np.zeros(max(int(nb.value), 1), dtype=np.uint8)
        off = np.zeros(max(n, 1), dtype=np.uint64)
        ln = np.zeros(max(n, 1), dtype=np.uint32)
        if n:
            gpu_check(self._g.kmpgpu_arena_download(self._ctx, a.ctypes.data, a.size, C.byref(nb), off.ctypes.data, ln.ctypes.data),
                      "kmpgpu_arena_download")
        return a[: int(nb.value)], off[:n], ln[:n]

    def arena_info(self) -> Tuple[int, int]:
        n, b = C.c_uint64(), C.c_uint64()
        gpu_check(self._g.kmpgpu_arena_info(self._ctx, C.byref(n), C.byref(b)), "kmpgpu_arena_info")
        return int(n.value), int(b.value)

    def effective_bytes(self) -> int:
        """Sum over payloads of min(len, first NUL + 1): what a strlen()-bounded scan (serial.c:191) has to
        touch; equals the payload bytes on NUL-free input."""
        b = C.c_uint64()
        gpu_check(self._g.kmpgpu_effective_bytes(self._ctx, C.byref(b)), "kmpgpu_effective_bytes")
        return int(b.value)

    # -- the hot path -----------------------------------------------------------------------------
    def scan(self) -> Tuple[np.ndarray, Timing]:
        """Per-pattern counts (uint64, pattern order) and the timing of this pass."""
        n = len(self.patterns)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        t = Timing()
        gpu_check(self._g.kmpgpu_scan(self._ctx, out.ctypes.data_as(u64p), C.byref(t)), "kmpgpu_scan")
        return out[:n], t

    def scan_enqueue(self, d_counts=None) -> None:
        """Enqueue one pass; counts land in d_counts (torch int64 CUDA tensor) or the context buffer."""
        ptr = d_counts.data_ptr() if d_counts is not None else None
        gpu_check(self._g.kmpgpu_scan_enqueue(self._ctx, ptr), "kmpgpu_scan_enqueue")

    def counts_read(self) -> np.ndarray:
        """Wait for the context's stream and read its own counts buffer (after scan_enqueue() / a count reduce)."""
        n = len(self.patterns)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        gpu_check(self._g.kmpgpu_counts_read(self._ctx, out.ctypes.data_as(u64p)), "kmpgpu_counts_read")
        return out[:n]

    def last_timing(self) -> Timing:
        t = Timing()
        gpu_check(self._g.kmpgpu_last_timing(self._ctx, C.byref(t)), "kmpgpu_last_timing")
        return t

    def counts_reset(self) -> None:
        gpu_check(self._g.kmpgpu_counts_reset(self._ctx), "kmpgpu_counts_reset")

    def sync(self) -> None:
        gpu_check(self._g.kmpgpu_sync(self._ctx), "kmpgpu_sync")

    def profile_begin(self, max_launches: int) -> None:
        gpu_check(self._g.kmpgpu_profile_begin(self._ctx, max_launches), "kmpgpu_profile_begin")

    def profile_end(self, max_launches: int) -> np.ndarray:
        ms = (C.c_float * max(max_launches, 1))()
        n = C.c_uint32()
        gpu_check(self._g.kmpgpu_profile_end(self._ctx, ms, C.byref(n)), "kmpgpu_profile_end")
        return np.array(ms[: n.value], dtype=np.float64)

    def scan_offsets(self, cap: int) -> Tuple[np.ndarray, int, np.ndarray]:
        """(matches[min(found,cap)] as a structured array, total found, counts)."""
        n = len(self.patterns)
        buf = (Match * max(cap, 1))()
        found = C.c_uint64()
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        gpu_check(self._g.kmpgpu_scan_offsets(self._ctx, buf, cap, C.byref(found), counts.ctypes.data_as(u64p)),
                  "kmpgpu_scan_offsets")
        k = min(int(found.value), cap)
        arr = np.frombuffer(buf, dtype=np.dtype([("packet", "<u8"), ("offset", "<u4"), ("pattern", "<u4")]), count=k).copy()
        return arr, int(found.value), counts[:n]

    def _scan_family(self, fn, rows: int, counts_key: str, hits: bool) -> dict:
        """What scan_packets, scan_rules, scan_relations, scan_chains, scan_headers, scan_bytetests and scan_regexes share: the C call ``fn`` over a family of ``rows`` rows, its
        per-row payload counts returned under ``counts_key``."""
        n = len(self.patterns)
        n_pkts, _ = self.arena_info()
        W = (n_pkts + 63) // 64
        row_counts = np.zeros(max(rows, 1), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        any_w = np.zeros(max(W, 1), dtype=np.uint64)
        hit_w = np.zeros((rows, W) if hits and rows * W else 1, dtype=np.uint64)
        t = Timing()
        gpu_check(getattr(self._g, fn)(self._ctx, row_counts.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data if hits else None,
                                       counts.ctypes.data, C.byref(t)), fn)
        out = {counts_key: row_counts[:rows], "counts": counts[:n], "timing": t,
               "any": np.unpackbits(any_w[:W].view(np.uint8), bitorder="little")[:n_pkts].astype(bool)}
        if hits:
            bits = np.unpackbits(hit_w.reshape(rows, W).view(np.uint8), axis=1, bitorder="little") if rows * W else np.zeros((rows, 0), np.uint8)
            out["hits"] = bits[:, :n_pkts].astype(bool)
        return out

    def scan_packets(self, hits: bool = False) -> dict:
        """Which payloads hold which patterns (kmpgpu_scan_packets), one pass on the device:
        ``pkt_counts`` (uint64[n_pat]) payloads that hold pattern i, ``any`` (bool[n_pkts]) payload k holds some pattern,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_pat, n_pkts])."""
        return self._scan_family("kmpgpu_scan_packets", len(self.patterns), "pkt_counts", hits)

    def scan_rules(self, hits: bool = False) -> dict:
        """Which payloads match which rules (kmpgpu_scan_rules): the marking pass of scan_packets and the rules on the device.
        ``rule_pkt_counts`` (uint64[n_rules]) payloads that rule r matches, ``any`` (bool[n_pkts]) payload k matches some rule,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_rules, n_pkts])."""
        return self._scan_family("kmpgpu_scan_rules", len(self.rules), "rule_pkt_counts", hits)

    def scan_flowbits(self, hits: bool = False, state: bool = False) -> dict:
        """The rules with their flow-bit ops over the built flows (kmpgpu_scan_flowbits): a dict as scan_rules returns -- its rows are the
        ALERT rows: fired, and no "noalert" on the rule --, plus ``flow_state`` (uint32[n_flows]) the state after every flow's last
        payload and, with state=True, ``state`` (bool[n_bits, n_pkts]): bit X before payload k."""
        n, rows, nb = len(self.patterns), len(self.rules), getattr(self, "n_flowbits", 0)
        n_pkts, _ = self.arena_info()
        n_flows = getattr(self, "_n_flows", 0)
        W = (n_pkts + 63) // 64
        row_counts = np.zeros(max(rows, 1), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        any_w = np.zeros(max(W, 1), dtype=np.uint64)
        hit_w = np.zeros((rows, W) if hits and rows * W else 1, dtype=np.uint64)
        st_w = np.zeros((nb, W) if state and nb * W else 1, dtype=np.uint64)
        flow_state = np.zeros(max(n_flows, 1), dtype=np.uint32)
        t = Timing()
        gpu_check(self._g.kmpgpu_scan_flowbits(self._ctx, row_counts.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data if hits else None,
                                               st_w.ctypes.data if state else None, flow_state.ctypes.data, counts.ctypes.data, C.byref(t)),
                  "kmpgpu_scan_flowbits")

        def unpack(words, r):
            bits = np.unpackbits(words.reshape(r, W).view(np.uint8), axis=1, bitorder="little") if r * W else np.zeros((r, 0), np.uint8)
            return bits[:, :n_pkts].astype(bool)
        out = {"rule_pkt_counts": row_counts[:rows], "counts": counts[:n], "timing": t, "flow_state": flow_state[:n_flows],
               "any": np.unpackbits(any_w[:W].view(np.uint8), bitorder="little")[:n_pkts].astype(bool)}
        if hits:
            out["hits"] = unpack(hit_w, rows)
        if state:
            out["state"] = unpack(st_w, nb)
        return out

    def scan_thresholds(self, ts, hits: bool = True, window_counts: bool = False) -> dict:
        """The rules with their rate thresholds (kmpgpu_scan_thresholds).  ts: one unsigned 64-bit timestamp per payload, in the unit of
        the thresholds' windows -- a numpy array, or a contiguous torch tensor of 64-bit integers on the matcher's device, handed over as
        it is.  A dict as scan_rules returns -- its rows are the ALERT rows --; with window_counts=True also ``window_counts``
        (uint32[n_thr, n_pkts]): the hits in payload k's tracker inside the window that ends at k, for every k."""
        n, rows, nq = len(self.patterns), len(self.rules), len(self.thresholds)
        n_pkts, _ = self.arena_info()
        on_device, keep = 0, None
        if isinstance(ts, np.ndarray) or not hasattr(ts, "is_cuda"):
            keep = np.asarray(ts)
            if keep.dtype.kind not in "ui" or (keep.dtype.kind == "i" and keep.size and int(keep.min()) < 0):
                raise ValueError(f"ts: non-negative integers are needed, not {keep.dtype}" + (" with negative values" if keep.dtype.kind == "i" else ""))
            keep = np.ascontiguousarray(keep.astype(np.uint64, copy=False)).reshape(-1)
            if keep.size != n_pkts:
                raise ValueError(f"ts: {keep.size} timestamps for {n_pkts} payloads")
            ptr = keep.ctypes.data if n_pkts else None
        else:                                     # a torch tensor
            if ts.dtype.itemsize != 8 or ts.dtype.is_floating_point or ts.numel() != n_pkts:
                raise ValueError(f"ts: a tensor of {n_pkts} 64-bit integers is needed")
            if ts.is_cuda:
                if ts.device.index != self.device or not ts.is_contiguous():
                    raise ValueError("ts: the tensor must be contiguous and on the matcher's device")
                import torch
                torch.cuda.current_stream(ts.device).synchronize()           # complete before the call (kmpgpu.h)
                on_device, ptr = 1, (ts.data_ptr() if n_pkts else None)
            else:
                keep = np.ascontiguousarray(ts.numpy()).view(np.uint64).reshape(-1)
                ptr = keep.ctypes.data if n_pkts else None
        W = (n_pkts + 63) // 64
        row_counts = np.zeros(max(rows, 1), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        any_w = np.zeros(max(W, 1), dtype=np.uint64)
        hit_w = np.zeros((rows, W) if hits and rows * W else 1, dtype=np.uint64)
        wc = np.zeros((nq, n_pkts) if window_counts and nq * n_pkts else 1, dtype=np.uint32)
        t = Timing()
        gpu_check(self._g.kmpgpu_scan_thresholds(self._ctx, ptr, on_device, row_counts.ctypes.data, any_w.ctypes.data,
                                                 hit_w.ctypes.data if hits else None, wc.ctypes.data if window_counts else None,
                                                 counts.ctypes.data, C.byref(t)), "kmpgpu_scan_thresholds")
        out = {"rule_pkt_counts": row_counts[:rows], "counts": counts[:n], "timing": t,
               "any": np.unpackbits(any_w[:W].view(np.uint8), bitorder="little")[:n_pkts].astype(bool)}
        if hits:
            bits = np.unpackbits(hit_w.reshape(rows, W).view(np.uint8), axis=1, bitorder="little") if rows * W else np.zeros((rows, 0), np.uint8)
            out["hits"] = bits[:, :n_pkts].astype(bool)
        if window_counts:
            out["window_counts"] = wc.reshape(nq, n_pkts) if nq * n_pkts else np.zeros((nq, n_pkts), np.uint32)
        return out

    def scan_relations(self, hits: bool = False) -> dict:
        """In which payloads which relations hold (kmpgpu_scan_relations): the marking pass of scan_packets and the relation kernel.
        ``rel_pkt_counts`` (uint64[n_rel]) payloads in which relation q holds, ``any`` (bool[n_pkts]) some relation holds in payload k,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_rel, n_pkts])."""
        return self._scan_family("kmpgpu_scan_relations", len(self.relations), "rel_pkt_counts", hits)

    def scan_chains(self, hits: bool = False) -> dict:
        """In which payloads which chains hold (kmpgpu_scan_chains): the marking pass of scan_packets and the chain kernel.
        ``chain_pkt_counts`` (uint64[n_chains]) payloads in which chain c holds, ``any`` (bool[n_pkts]) some chain holds in payload k,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_chains, n_pkts])."""
        return self._scan_family("kmpgpu_scan_chains", len(self.chains), "chain_pkt_counts", hits)

    def scan_headers(self, hits: bool = False) -> dict:
        """For which payloads which header predicates hold (kmpgpu_scan_headers): the marking pass of scan_packets and the header kernel.
        ``hdr_pkt_counts`` (uint64[n_hdr]) payloads for which predicate q holds, ``any`` (bool[n_pkts]) some predicate holds for payload k,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_hdr, n_pkts])."""
        return self._scan_family("kmpgpu_scan_headers", len(self.headers), "hdr_pkt_counts", hits)

    def scan_bytetests(self, hits: bool = False) -> dict:
        """For which payloads which byte tests hold (kmpgpu_scan_bytetests): the marking pass of scan_packets and the byte-test kernels.
        ``bt_pkt_counts`` (uint64[n_bt]) payloads for which test q holds, ``any`` (bool[n_pkts]) some test holds for payload k,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_bt, n_pkts])."""
        return self._scan_family("kmpgpu_scan_bytetests", len(self.bytetests), "bt_pkt_counts", hits)

    def scan_regexes(self, hits: bool = False) -> dict:
        """Which payloads which expressions hit (kmpgpu_scan_regexes): the marking pass of scan_packets and the regex kernel.
        ``rx_pkt_counts`` (uint64[n_rx]) payloads that expression q hits, ``any`` (bool[n_pkts]) some expression hits payload k,
        ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[n_rx, n_pkts])."""
        return self._scan_family("kmpgpu_scan_regexes", len(self.regexes), "rx_pkt_counts", hits)

    def scan_alerts(self, family: str = "rules", max_records: Optional[int] = None, read: bool = True) -> dict:
        """Which payloads hit which rows of a family, as a list built on the device (kmpgpu_scan_alerts): family "patterns", "rules",
        "relations" or "chains" -- the rows of scan_packets, scan_rules, scan_relations, scan_chains.  ``n_found`` the length of the
        whole list, ``n_packets`` the distinct payloads in it, ``pkt_counts`` (uint64[rows]) what the family's own call returns under
        its name for it, ``counts`` (uint64[n_pat]) as scan(), ``timing``, and ``alerts``: the kept prefix -- the first
        min(max_records, n_found) records of the list sorted by packet, then index; max_records None keeps all -- as a structured
        array (ALERT_DTYPE), or with read=False an empty one: the records stay on the device for alerts_read()."""
        if family not in ALERT_FAMILIES:
            raise ValueError(f"family {family!r}: one of {sorted(ALERT_FAMILIES)} is needed")
        cap = ALERTS_ALL if max_records is None else int(max_records)
        if not 0 <= cap <= ALERTS_ALL:
            raise ValueError(f"max_records {max_records}: not a 64-bit count")
        n = len(self.patterns)
        rows = {"patterns": n, "rules": len(self.rules), "relations": len(self.relations), "chains": len(self.chains)}[family]
        found, packets = C.c_uint64(), C.c_uint64()
        pkt_counts = np.zeros(max(rows, 1), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        t = Timing()
        gpu_check(self._g.kmpgpu_scan_alerts(self._ctx, ALERT_FAMILIES[family], cap, C.byref(found), C.byref(packets), pkt_counts.ctypes.data,
                                             counts.ctypes.data, C.byref(t)), "kmpgpu_scan_alerts")
        kept = min(int(found.value), cap)
        return {"alerts": self.alerts_read(0, kept) if read else np.zeros(0, dtype=ALERT_DTYPE), "n_found": int(found.value),
                "n_packets": int(packets.value), "pkt_counts": pkt_counts[:rows], "counts": counts[:n], "timing": t}

    def alerts_read(self, first: int, n: int) -> np.ndarray:
        """Records [first, first + n) of the prefix the last scan_alerts kept on the device (kmpgpu_alerts_read)."""
        out = np.zeros(max(int(n), 1), dtype=ALERT_DTYPE)
        gpu_check(self._g.kmpgpu_alerts_read(self._ctx, out.ctypes.data, int(first), int(n)), "kmpgpu_alerts_read")
        return out[: int(n)]

    # -- flows ------------------------------------------------------------------------------------
    def build_flows(self, directed: bool = False) -> int:
        """Group the arena's payloads by the 5-tuple of their metadata, on the device (kmpgpu_flows_build): both directions of a
        conversation are one flow unless ``directed``.  Returns the number of flows; they are numbered in the order of their first
        payload and stay until the arena or its metadata change."""
        n = C.c_uint64()
        gpu_check(self._g.kmpgpu_flows_build(self._ctx, FLOW_DIRECTED if directed else 0, C.byref(n), None), "kmpgpu_flows_build")
        self._n_flows = int(n.value)
        return self._n_flows

    def flows(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records [first, first + n) of the flows (kmpgpu_flows_read) as a FLOW_DTYPE array; n None: all from ``first`` on."""
        n = self._flow_count() - int(first) if n is None else int(n)
        out = np.zeros(max(n, 1), dtype=FLOW_DTYPE)
        gpu_check(self._g.kmpgpu_flows_read(self._ctx, out.ctypes.data, int(first), max(n, 0)), "kmpgpu_flows_read")
        return out[: max(n, 0)]

    def flow_ids(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """flow_of[first .. first + n) (kmpgpu_flow_ids_read), uint32; n None: all from ``first`` on."""
        n = self.arena_info()[0] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        gpu_check(self._g.kmpgpu_flow_ids_read(self._ctx, out.ctypes.data, int(first), max(n, 0)), "kmpgpu_flow_ids_read")
        return out[: max(n, 0)]

    def _flow_count(self) -> int:
        """The flows the context holds; KmpGpuError where it has none (the library is asked: it knows when they were dropped)."""
        gpu_check(self._g.kmpgpu_flows_read(self._ctx, None, 0, 0), "kmpgpu_flows_read")
        return getattr(self, "_n_flows", 0)

    def scan_flows(self, family: str = "rules", scope: str = "packet", hits: bool = False) -> dict:
        """The rows of a family in flow space (kmpgpu_scan_flows).  scope "packet": flow f is in row r where one of its payloads is in
        row r of the family's own call; scope "flow" (rules only): every term row is folded first and the rule evaluated per flow -- its
        contents may lie in different payloads of the connection.  ``flow_counts`` (uint64[rows]) flows in row r, ``any``
        (bool[n_flows]), ``counts`` (uint64[n_pat]) as scan(), ``timing``; with hits=True also ``hits`` (bool[rows, n_flows])."""
        if family not in ALERT_FAMILIES:
            raise ValueError(f"family {family!r}: one of {sorted(ALERT_FAMILIES)} is needed")
        if scope not in FLOW_SCOPES:
            raise ValueError(f"scope {scope!r}: one of {sorted(FLOW_SCOPES)} is needed")
        rows = {"patterns": len(self.patterns), "rules": len(self.rules), "relations": len(self.relations), "chains": len(self.chains)}[family]

        def call(row_counts, any_w, hit_w, counts, t):
            return self._g.kmpgpu_scan_flows(self._ctx, ALERT_FAMILIES[family], FLOW_SCOPES[scope], row_counts, any_w, hit_w, counts, t)
        return self._scan_flow_rows(call, "kmpgpu_scan_flows", rows, hits)

    def _scan_flow_rows(self, call, name: str, rows: int, hits: bool) -> dict:
        """What scan_flows and scan_flow_seams share: the output buffers of a flow-space call and their unpacking."""
        n = len(self.patterns)
        n_flows = getattr(self, "_n_flows", 0)
        Wf = (n_flows + 63) // 64
        row_counts = np.zeros(max(rows, 1), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        any_w = np.zeros(max(Wf, 1), dtype=np.uint64)
        hit_w = np.zeros((rows, Wf) if hits and rows * Wf else 1, dtype=np.uint64)
        t = Timing()
        gpu_check(call(row_counts.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data if hits else None, counts.ctypes.data, C.byref(t)), name)
        out = {"flow_counts": row_counts[:rows], "counts": counts[:n], "timing": t,
               "any": np.unpackbits(any_w[:Wf].view(np.uint8), bitorder="little")[:n_flows].astype(bool)}
        if hits:
            bits = np.unpackbits(hit_w.reshape(rows, Wf).view(np.uint8), axis=1, bitorder="little") if rows * Wf else np.zeros((rows, 0), np.uint8)
            out["hits"] = bits[:, :n_flows].astype(bool)
        return out

    # -- flow seams --------------------------------------------------------------------------------
    def load_seams(self, src: "GpuMatcher", reach: int = 98) -> int:
        """Make this matcher's arena the seams of ``src``, whose flows are built (kmpgpu_load_seams): for every payload with a predecessor
        in its flow and direction, the predecessor's last ``reach`` bytes followed by the payload's first ``reach`` bytes, as a payload of
        its own.  A pattern of up to reach + 1 bytes that straddles the boundary lies inside the seam.  Patterns, rules, windows and options
        of this matcher stay.  Returns the number of seams."""
        n = C.c_uint64()
        gpu_check(self._g.kmpgpu_load_seams(self._ctx, src._ctx, int(reach), C.byref(n)), "kmpgpu_load_seams")
        self._keep = None
        self._n_seams = int(n.value)
        return self._n_seams

    def seams(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records [first, first + n) of the seam list (kmpgpu_seams_read) as a SEAM_DTYPE array; n None: all from ``first`` on."""
        gpu_check(self._g.kmpgpu_seams_read(self._ctx, None, 0, 0), "kmpgpu_seams_read")        # (the library knows when the list was dropped)
        n = getattr(self, "_n_seams", 0) - int(first) if n is None else int(n)
        out = np.zeros(max(n, 1), dtype=SEAM_DTYPE)
        gpu_check(self._g.kmpgpu_seams_read(self._ctx, out.ctypes.data, int(first), max(n, 0)), "kmpgpu_seams_read")
        return out[: max(n, 0)]

    def scan_flow_seams(self, seams: "GpuMatcher", hits: bool = False) -> dict:
        """scan_flows("rules", "flow") with the pattern rows of ``seams`` -- a matcher that holds this one's patterns and the seam list
        load_seams built from this one's current flows -- folded into the term rows (kmpgpu_scan_flows_seams): a content split across two
        consecutive payloads of a flow direction counts as present in the flow.  The result is shaped like scan_flows'."""
        def call(row_counts, any_w, hit_w, counts, t):
            return self._g.kmpgpu_scan_flows_seams(self._ctx, seams._ctx, row_counts, any_w, hit_w, counts, t)
        return self._scan_flow_rows(call, "kmpgpu_scan_flows_seams", len(self.rules), hits)

    # -- flow streams ------------------------------------------------------------------------------
    def load_streams(self, src: "GpuMatcher", depth: int = 1 << 20, seq=None) -> int:
        """Make this matcher's arena the reassembled streams of ``src``, whose flows are built (kmpgpu_load_streams): the payloads of
        every (flow, direction) concatenated in capture order and cut to ``depth`` bytes, as one payload each, numbered by
        flow << 1 | dir.  Every scan of this matcher then sees a content however it was cut into segments; build_flows() here, with the
        flag ``src``'s flows were built with, reproduces ``src``'s flow numbering.  Patterns, rules, windows and options of this matcher
        stay.  Returns the number of streams.

        seq: one 32-bit TCP sequence number per payload of ``src`` -- a numpy array, or a contiguous torch tensor of 32-bit integers on
        ``src``'s device, handed over as it is -- builds the TCP streams in sequence order instead (kmpgpu_load_streams_ordered):
        retransmitted bytes dropped, holes closed; stream_segs() and stream_orders() then say what was kept."""
        n = C.c_uint64()
        if seq is None:
            gpu_check(self._g.kmpgpu_load_streams(self._ctx, src._ctx, int(depth), C.byref(n)), "kmpgpu_load_streams")
        else:
            n_src, _ = src.arena_info()
            on_device = 0
            if isinstance(seq, np.ndarray) or not hasattr(seq, "is_cuda"):
                words = np.ascontiguousarray(np.asarray(seq).astype(np.uint32, copy=False)).reshape(-1)
                if words.size != n_src:
                    raise ValueError(f"seq: {words.size} sequence numbers for {n_src} payloads")
                ptr = words.ctypes.data if n_src else None
            else:                                 # a torch tensor
                if seq.dtype.itemsize != 4 or seq.dtype.is_floating_point or seq.numel() != n_src:
                    raise ValueError(f"seq: a tensor of {n_src} 32-bit integers is needed")
                if seq.is_cuda:
                    if seq.device.index != src.device or not seq.is_contiguous():
                        raise ValueError("seq: the tensor must be contiguous and on the source's device")
                    import torch
                    torch.cuda.current_stream(seq.device).synchronize()      # complete before the call (kmpgpu.h)
                    on_device, ptr = 1, (seq.data_ptr() if n_src else None)
                else:
                    words = np.ascontiguousarray(seq.numpy()).view(np.uint32).reshape(-1)
                    ptr = words.ctypes.data if n_src else None
            gpu_check(self._g.kmpgpu_load_streams_ordered(self._ctx, src._ctx, int(depth), ptr, on_device, C.byref(n)),
                      "kmpgpu_load_streams_ordered")
        self._keep = None
        self._n_streams = int(n.value)
        self._n_stream_map = src.arena_info()[0]
        return self._n_streams

    def _stream_read(self, fn, name: str, total: str, dtype, first: int, n: Optional[int]) -> np.ndarray:
        gpu_check(fn(self._ctx, None, 0, 0), name)                           # (the library knows when the records were dropped)
        n = getattr(self, total, 0) - int(first) if n is None else int(n)
        out = np.zeros(max(n, 1), dtype=dtype)
        gpu_check(fn(self._ctx, out.ctypes.data, int(first), max(n, 0)), name)
        return out[: max(n, 0)]

    def streams(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records [first, first + n) of the streams (kmpgpu_streams_read) as a STREAM_DTYPE array; n None: all from ``first`` on."""
        return self._stream_read(self._g.kmpgpu_streams_read, "kmpgpu_streams_read", "_n_streams", STREAM_DTYPE, first, n)

    def stream_map(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Entries [first, first + n) of the map (kmpgpu_stream_map_read), one per payload of the source, as a STREAM_POS_DTYPE array;
        n None: all from ``first`` on.  stream_locate() maps offsets in streams back through it."""
        return self._stream_read(self._g.kmpgpu_stream_map_read, "kmpgpu_stream_map_read", "_n_stream_map", STREAM_POS_DTYPE, first, n)

    def stream_segs(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Entries [first, first + n) of what load_streams(seq=...) kept of every payload of the source (kmpgpu_stream_segs_read) as a
        STREAM_SEG_DTYPE array; n None: all from ``first`` on.  stream_locate_ordered() maps offsets in streams back through it."""
        return self._stream_read(self._g.kmpgpu_stream_segs_read, "kmpgpu_stream_segs_read", "_n_stream_map", STREAM_SEG_DTYPE, first, n)

    def stream_orders(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Records [first, first + n) of the streams' sequence order (kmpgpu_stream_orders_read) as a STREAM_ORDER_DTYPE array: the
        lowest sequence number, gaps and dropped bytes; n None: all from ``first`` on."""
        return self._stream_read(self._g.kmpgpu_stream_orders_read, "kmpgpu_stream_orders_read", "_n_streams", STREAM_ORDER_DTYPE, first, n)

    def select_flows(self, bits, device: bool = False):
        """The payloads of the chosen flows as a payload bitmap (kmpgpu_flows_select): bits is bool[n_flows] or uint64[ceil(n_flows / 64)]
        on the host, or a torch tensor of that many 64-bit words on this matcher's device.  Returns uint64[ceil(n_pkts / 64)] words as
        load_selected takes them; with device=True a torch int64 tensor of them on the device instead, copied from the context's buffer."""
        n_flows = self._flow_count()
        n_pkts, _ = self.arena_info()
        W, Wf = (n_pkts + 63) // 64, (n_flows + 63) // 64
        on_device = 0
        if isinstance(bits, np.ndarray):
            words = select_words(bits, n_flows)
            ptr = words.ctypes.data if Wf else None
        else:                                     # a torch tensor
            if bits.dtype.itemsize != 8 or bits.dtype.is_floating_point or bits.numel() != Wf or not bits.is_cuda \
                    or bits.device.index != self.device or not bits.is_contiguous():
                raise ValueError(f"bits: a contiguous tensor of {Wf} 64-bit words on the matcher's device is needed for {n_flows} flows")
            import torch
            torch.cuda.current_stream(bits.device).synchronize()             # complete before the call (kmpgpu.h)
            on_device, ptr = 1, (bits.data_ptr() if Wf else None)
        out = np.zeros(max(W, 1), dtype=np.uint64)
        d_ptr = C.c_void_p()
        gpu_check(self._g.kmpgpu_flows_select(self._ctx, ptr, on_device, None if device else out.ctypes.data, C.byref(d_ptr)),
                  "kmpgpu_flows_select")
        if not device:
            return out[:W]
        import torch
        if not W:
            return torch.zeros(0, dtype=torch.int64, device=f"cuda:{self.device}")

        class _Words:                             # the context's buffer, as torch reads foreign device memory
            __cuda_array_interface__ = {"shape": (W,), "typestr": "<i8", "data": (int(d_ptr.value), False), "version": 2}
        # the buffer holds until the next select_flows: a copy of the caller's own outlives it
        return torch.as_tensor(_Words(), device=f"cuda:{self.device}").clone()

    # -- synthetic input (bench / tests) ---------------------------------------------------------
    def synth_fill(self, d_arena, d_off, d_len, sp: SynthParams, first_pkt_id: int = 0) -> None:
        gpu_check(self._g.kmpgpu_synth_fill(self._ctx, d_arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), first_pkt_id,
                                            int(d_len.numel()), C.byref(sp)), "kmpgpu_synth_fill")

    def fixed_index(self, d_off, d_len, length: int, slot_align: int = 16) -> None:
        gpu_check(self._g.kmpgpu_fixed_index(self._ctx, d_off.data_ptr(), d_len.data_ptr(), int(d_len.numel()), length,
                                             slot_align), "kmpgpu_fixed_index")

    # -- lifetime ----------------------------------------------------------------------------------
    def close(self) -> None:
        comm = getattr(self, "_comm", None)
        if comm is not None:                      # the communicator goes before its contexts (kmpgpu.h)
            self._comm = None
            comm.close()
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._g.kmpgpu_destroy(self._ctx)
            self._ctx = C.c_void_p()
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class GpuComm:
    """RCCL count reduce behind the C-ABI (kmpgpu_comm_*): replaces MPI_Reduce(..., MPI_SUM ...) of mpi_dumping.c:202.

    ``GpuComm(matchers)``: all ranks in this process, one matcher per device (ncclCommInitAll).
    ``GpuComm.from_rank(matcher, n_ranks, rank, unique_id)``: one process per GPU; ``GpuComm.unique_id()`` makes the id."""

    def __init__(self, matchers: Sequence["GpuMatcher"]):
        self._g = _lib.gpu_lib()
        self._comm = C.c_void_p()
        self._matchers = list(matchers)
        arr = (C.c_void_p * len(self._matchers))(*[m._ctx for m in self._matchers])
        gpu_check(self._g.kmpgpu_comm_init(C.byref(self._comm), arr, len(self._matchers)), "kmpgpu_comm_init")
        for m in self._matchers:
            m._comm = self

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        gpu_check(_lib.gpu_lib().kmpgpu_comm_unique_id(buf), "kmpgpu_comm_unique_id")
        return buf.raw

    @classmethod
    def from_rank(cls, matcher: "GpuMatcher", n_ranks: int, rank: int, unique_id: bytes) -> "GpuComm":
        self = cls.__new__(cls)
        self._g = _lib.gpu_lib()
        self._comm = C.c_void_p()
        self._matchers = [matcher]
        gpu_check(self._g.kmpgpu_comm_init_rank(C.byref(self._comm), matcher._ctx, n_ranks, rank, C.c_char_p(unique_id)), "kmpgpu_comm_init_rank")
        matcher._comm = self
        return self

    def allreduce_counts(self) -> None:
        gpu_check(self._g.kmpgpu_comm_allreduce_counts(self._comm), "kmpgpu_comm_allreduce_counts")

    def close(self) -> None:
        if getattr(self, "_comm", None) is not None and self._comm.value:
            self._g.kmpgpu_comm_destroy(self._comm)
            self._comm = C.c_void_p()
        for m in getattr(self, "_matchers", []):
            if getattr(m, "_comm", None) is self:
                m._comm = None
        self._matchers = []

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def count_matches(patterns: Sequence[bytes], arena: HostArena, device: int = 0, nocase=False, whole_payload=False, **options) -> np.ndarray:
    """One-shot helper: counts of every pattern over a host arena on one GPU (nocase: as GpuMatcher.set_patterns;
    whole_payload: payloads are text up to their ends, OPT_WHOLE_PAYLOAD, instead of up to their first 0x00)."""
    with GpuMatcher(device) as m:
        for k, v in options.items():
            m.set_option({"mode": OPT_MODE, "depth": OPT_DEPTH, "blocks_per_cu": OPT_BLOCKS_PER_CU}[k], v)
        if whole_payload:
            m.set_option(OPT_WHOLE_PAYLOAD, 1)
        m.set_patterns(patterns, nocase=nocase)
        m.load_arena(arena)
        return m.scan()[0]
