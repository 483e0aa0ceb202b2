"""Python view of the C host library (include/kmphost.h).  No GPU needed.

Used by the tests, the benchmark and the smoke check to drive exactly the host code the CLI
programs (bin/serial, bin/openmp_data) run: pcap savefile reader, payload extraction, pattern
loader, arena builder.  Reference citations are relative to the reference repository.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Arena, KmpHostError, Patterns, SynthParams, u8p, u32p, u64p

PROTO = {"udp": 0, "tcp": 1}
# kmp_pkt_meta / kmpgpu_pkt_meta, 16 bytes: what GpuMatcher.set_meta takes and .meta() returns
META_DTYPE = np.dtype([("src_ip", "<u4"), ("dst_ip", "<u4"), ("src_port", "<u2"), ("dst_port", "<u2"), ("proto", "u1"), ("reserved", "u1", (3,))])
# kmp_header / kmpgpu_header, 36 bytes: one header predicate
# kmp_bytetest / kmpgpu_bytetest, 20 bytes: one byte test
BYTETEST_DTYPE = np.dtype([("anchor", "<u4"), ("offset", "<i4"), ("mask", "<u4"), ("value", "<u4"), ("nbytes", "u1"), ("op", "u1"), ("flags", "u1"),
                           ("reserved", "u1")])
HEADER_DTYPE = np.dtype([("src_ip", "<u4"), ("src_mask", "<u4"), ("dst_ip", "<u4"), ("dst_mask", "<u4"), ("sport_lo", "<u2"), ("sport_hi", "<u2"),
                         ("dport_lo", "<u2"), ("dport_hi", "<u2"), ("len_lo", "<u4"), ("len_hi", "<u4"), ("proto", "u1"), ("flags", "u1"),
                         ("reserved", "<u2")])


def _np_ptr(a: np.ndarray, t):
    return a.ctypes.data_as(t)


# ---------------------------------------------------------------------------------------------
# patterns  (serial.c:54-87)
# ---------------------------------------------------------------------------------------------
def _patterns_to_list(p: Patterns) -> List[bytes]:
    out = []
    for i in range(p.n):
        out.append(C.string_at(C.addressof(p.blob.contents) + p.off[i], p.len[i]))
    return out


def load_patterns(path: str) -> List[bytes]:
    """Tokens of a pattern file in file order, duplicates kept (fscanf("%s"), serial.c:66)."""
    L = _lib.host_lib()
    p = Patterns()
    rc = L.kmp_patterns_load(path.encode(), C.byref(p))
    if rc:
        raise KmpHostError(f"kmp_patterns_load({path}) failed: {rc}")
    try:
        return _patterns_to_list(p)
    finally:
        L.kmp_patterns_free(C.byref(p))


def parse_patterns(text: bytes) -> List[bytes]:
    L = _lib.host_lib()
    p = Patterns()
    buf = np.frombuffer(text + b"\0", dtype=np.uint8).copy()
    rc = L.kmp_patterns_parse(_np_ptr(buf, u8p), len(text), C.byref(p))
    if rc:
        raise KmpHostError(f"kmp_patterns_parse failed: {rc}")
    try:
        return _patterns_to_list(p)
    finally:
        L.kmp_patterns_free(C.byref(p))


def failure_table(pat: bytes) -> List[int]:
    """KMP failure function (kmp_prefix, serial.c:217-238)."""
    L = _lib.host_lib()
    b = np.frombuffer(pat + b"\0", dtype=np.uint8).copy()
    out = np.zeros(max(len(pat), 1), dtype=np.int32)
    L.kmp_failure_table(_np_ptr(b, u8p), len(pat), _np_ptr(out, _lib.i32p))
    return out[: len(pat)].tolist()


# ---------------------------------------------------------------------------------------------
# pcap + extraction  (serial.c:91,115 ; packet_dumping.h:87-188)
# ---------------------------------------------------------------------------------------------
def read_pcap(path: str) -> Iterator[Tuple[int, int, bytes]]:
    """(caplen, len, frame) for every record of a classic pcap savefile."""
    L = _lib.host_lib()
    err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
    h = L.kmp_pcap_open(path.encode(), err)
    if not h:
        raise KmpHostError(f"error reading pcap file: {err.value.decode(errors='replace')}")
    try:
        cl, ln, data = C.c_uint32(), C.c_uint32(), u8p()
        while L.kmp_pcap_next(h, C.byref(cl), C.byref(ln), C.byref(data)) >= 0:
            yield cl.value, ln.value, C.string_at(data, cl.value)
    finally:
        L.kmp_pcap_close(h)


def extract(frame: bytes, capture_len: Optional[int] = None, proto: str = "udp") -> Optional[Tuple[int, int]]:
    """(payload offset, payload length) or None (dump_UDP_packet / dump_TCP_packet)."""
    L = _lib.host_lib()
    buf = np.frombuffer(frame + b"\0" * 64, dtype=np.uint8).copy()
    off, ln = C.c_uint32(), C.c_uint32()
    fn = L.kmp_extract_udp if proto == "udp" else L.kmp_extract_tcp
    cl = len(frame) if capture_len is None else capture_len
    ok = fn(_np_ptr(buf, u8p), cl, C.byref(off), C.byref(ln))
    return (off.value, ln.value) if ok else None


def extract_meta(frame: bytes, capture_len: Optional[int] = None, proto: str = "udp") -> Optional[np.ndarray]:
    """The header fields of a frame the extractor of `proto` accepts, as a META_DTYPE scalar, or None (kmp_extract_meta)."""
    L = _lib.host_lib()
    buf = np.frombuffer(frame + b"\0" * 64, dtype=np.uint8).copy()
    m = _lib.PktMeta()
    cl = len(frame) if capture_len is None else capture_len
    if not L.kmp_extract_meta(_np_ptr(buf, u8p), cl, PROTO[proto], C.byref(m)):
        return None
    return np.frombuffer(bytes(m), dtype=META_DTYPE)[0]


def parse_headers(path: str) -> np.ndarray:
    """The predicates of a headers file as a HEADER_DTYPE array (kmp_headers_parse); KmpHostError carries the parser's message."""
    L = _lib.host_lib()
    h = _lib.Headers()
    err = C.create_string_buffer(_lib.KMP_HEADERS_ERRBUF)
    rc = L.kmp_headers_parse(path.encode(), C.byref(h), err)
    if rc:
        raise KmpHostError(f"{err.value.decode(errors='replace')} ({rc})")
    try:
        return np.frombuffer(C.string_at(h.hdr, h.n * C.sizeof(_lib.Header)), dtype=HEADER_DTYPE).copy() if h.n else np.zeros(0, HEADER_DTYPE)
    finally:
        L.kmp_headers_free(C.byref(h))


def parse_bytetests(path: str, n_patterns: int) -> np.ndarray:
    """The tests of a byte tests file as a BYTETEST_DTYPE array (kmp_bytetests_parse); KmpHostError carries the parser's message."""
    L = _lib.host_lib()
    b = _lib.ByteTests()
    err = C.create_string_buffer(_lib.KMP_BYTETESTS_ERRBUF)
    rc = L.kmp_bytetests_parse(path.encode(), n_patterns, C.byref(b), err)
    if rc:
        raise KmpHostError(f"{err.value.decode(errors='replace')} ({rc})")
    try:
        return np.frombuffer(C.string_at(b.bt, b.n * C.sizeof(_lib.ByteTest)), dtype=BYTETEST_DTYPE).copy() if b.n else np.zeros(0, BYTETEST_DTYPE)
    finally:
        L.kmp_bytetests_free(C.byref(b))


def parse_regexes(path: str, n_patterns: int) -> list:
    """The expressions of an expressions file as GpuMatcher.set_regexes takes them (kmp_regexes_parse): (bytes, dict) per line, the dict
    with nocase, dotall and gate where the line has them; KmpHostError carries the parser's message."""
    L = _lib.host_lib()
    r = _lib.Regexes()
    err = C.create_string_buffer(_lib.KMP_REGEXES_ERRBUF)
    rc = L.kmp_regexes_parse(path.encode(), n_patterns, C.byref(r), err)
    if rc:
        raise KmpHostError(f"{err.value.decode(errors='replace')} ({rc})")
    try:
        out = []
        for q in range(r.n):
            opt = {}
            if r.flags[q] & _lib.RX_NOCASE:
                opt["nocase"] = True
            if r.flags[q] & _lib.RX_DOTALL:
                opt["dotall"] = True
            if r.flags[q] & _lib.RX_GROUPS:
                opt["groups"] = True
            if r.flags[q] & _lib.RX_GATED:
                opt["gate"] = int(r.gate[q])
            out.append((C.string_at(r.expr[q], r.len[q]), opt))
        return out
    finally:
        L.kmp_regexes_free(C.byref(r))


# ---------------------------------------------------------------------------------------------
# arena  (replaces char **array_of_payloads, serial.c:99,124-136)
# ---------------------------------------------------------------------------------------------
class HostArena:
    """One contiguous payload arena + {offset, length} index, 16-byte aligned slots."""

    def __init__(self, arena: Arena, owner: bool = True, meta: Optional[np.ndarray] = None, seq: Optional[np.ndarray] = None,
                 ts: Optional[np.ndarray] = None):
        self._a = arena
        self._owner = owner
        self.meta = meta           # META_DTYPE[n_pkts] where the arena was built with_meta, else None
        self.seq = seq             # uint32[n_pkts] where the arena was built with_seq, else None
        self.ts = ts               # uint64[n_pkts], microseconds, where the arena was built with_ts, else None
        n = int(arena.n_pkts)
        self.n_pkts = n
        self.n_frames = int(arena.n_frames)
        self.payload_bytes = int(arena.payload_bytes)
        self.nbytes = int(arena.nbytes)
        self.bytes = np.ctypeslib.as_array(arena.bytes, shape=(self.nbytes,)) if self.nbytes else np.zeros(0, np.uint8)
        self.off = np.ctypeslib.as_array(arena.off, shape=(max(n, 1),))[:n]
        self.len = np.ctypeslib.as_array(arena.len, shape=(max(n, 1),))[:n]

    @classmethod
    def from_pcap(cls, path: str, proto: str = "udp", pinned: bool = False, with_meta: bool = False, with_seq: bool = False,
                  with_ts: bool = False) -> "HostArena":
        """serial.c:115-141: read every record, extract, store (invalid frames skipped).  with_meta: the identical arena, and in
        ``.meta`` the accepted frames' header fields in payload order (kmp_arena_from_pcap_meta), as GpuMatcher.set_meta takes them.
        with_seq: in ``.seq`` their TCP sequence numbers (kmp_arena_from_pcap_seq), as GpuMatcher.load_streams(seq=...) takes them.
        with_ts: in ``.ts`` their capture times in microseconds (kmp_arena_from_pcap_ts), as GpuMatcher.scan_thresholds takes them."""
        L = _lib.host_lib()
        a = Arena()
        err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
        alloc = free = None
        if pinned:
            g = _lib.gpu_lib()
            alloc = C.cast(g.kmpgpu_host_alloc, C.c_void_p)
            free = C.cast(g.kmpgpu_host_free, C.c_void_p)
        mp = C.POINTER(_lib.PktMeta)()
        sp, tp = _lib.u32p(), _lib.u64p()
        if with_ts:
            rc = L.kmp_arena_from_pcap_seq_ts(path.encode(), PROTO[proto], alloc, free, C.byref(a), err, C.byref(mp) if with_meta else None,
                                              C.byref(sp) if with_seq else None, C.byref(tp))
        elif with_seq:
            rc = L.kmp_arena_from_pcap_seq(path.encode(), PROTO[proto], alloc, free, C.byref(a), err, C.byref(mp) if with_meta else None,
                                           C.byref(sp))
        elif with_meta:
            rc = L.kmp_arena_from_pcap_meta(path.encode(), PROTO[proto], alloc, free, C.byref(a), err, C.byref(mp))
        else:
            rc = L.kmp_arena_from_pcap(path.encode(), PROTO[proto], alloc, free, C.byref(a), err)
        if rc:
            raise KmpHostError(f"error reading pcap file: {err.value.decode(errors='replace')} ({rc})")
        meta = None
        if with_meta:
            meta = np.frombuffer(C.string_at(mp, int(a.n_pkts) * 16), dtype=META_DTYPE).copy() if a.n_pkts else np.zeros(0, META_DTYPE)
            C.CDLL(None).free(C.cast(mp, C.c_void_p))       # (malloc'ed by the library, kmphost.h)
        seq = None
        if with_seq:
            seq = np.frombuffer(C.string_at(sp, int(a.n_pkts) * 4), dtype=np.uint32).copy() if a.n_pkts else np.zeros(0, np.uint32)
            C.CDLL(None).free(C.cast(sp, C.c_void_p))
        ts = None
        if with_ts:
            ts = np.frombuffer(C.string_at(tp, int(a.n_pkts) * 8), dtype=np.uint64).copy() if a.n_pkts else np.zeros(0, np.uint64)
            C.CDLL(None).free(C.cast(tp, C.c_void_p))
        return cls(a, meta=meta, seq=seq, ts=ts)

    @classmethod
    def from_payloads(cls, payloads: Sequence[bytes]) -> "HostArena":
        L = _lib.host_lib()
        n = len(payloads)
        keep = [np.frombuffer(p + b"\0", dtype=np.uint8) for p in payloads]
        ptrs = (u8p * max(n, 1))(*[_np_ptr(k, u8p) for k in keep])
        lens = np.array([len(p) for p in payloads], dtype=np.uint32) if n else np.zeros(1, np.uint32)
        a = Arena()
        rc = L.kmp_arena_from_payloads(ptrs, _np_ptr(lens, u32p), n, None, None, C.byref(a))
        if rc:
            raise KmpHostError(f"kmp_arena_from_payloads failed: {rc}")
        return cls(a)

    def payload(self, k: int) -> bytes:
        o, l = int(self.off[k]), int(self.len[k])
        return self.bytes[o:o + l].tobytes()

    def close(self) -> None:
        if self._owner and self._a is not None:
            self.bytes = self.off = self.len = None
            _lib.host_lib().kmp_arena_free(C.byref(self._a))
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def arena_layout(lens: Optional[np.ndarray], fixed_len: int, n: int, slot_align: int = 16) -> Tuple[np.ndarray, np.ndarray, int]:
    """(off u64[n], len u32[n], arena bytes incl. slack) for given or fixed payload lengths."""
    L = _lib.host_lib()
    off = np.zeros(max(n, 1), dtype=np.uint64)
    ln = np.zeros(max(n, 1), dtype=np.uint32)
    lp = _np_ptr(np.ascontiguousarray(lens, dtype=np.uint32), u32p) if lens is not None else None
    nbytes = L.kmp_arena_layout(lp, fixed_len, n, slot_align, _np_ptr(off, u64p), _np_ptr(ln, u32p))
    return off[:n], ln[:n], int(nbytes)


def synth_fill_host(arena: np.ndarray, off: np.ndarray, ln: np.ndarray, sp: SynthParams, first_pkt_id: int = 0,
                    threads: int = 1) -> None:
    """Synthetic payloads on the host -- same bytes as the device generator (include/kmp_synth.h)."""
    L = _lib.host_lib()
    L.kmp_synth_fill_host(_np_ptr(arena, u8p), _np_ptr(off, u64p), _np_ptr(ln, u32p), first_pkt_id, len(ln), C.byref(sp), threads)


def synth_count_planted(sp: SynthParams, n: int, fixed_len: int = 0, lens: Optional[np.ndarray] = None, first_pkt_id: int = 0) -> int:
    L = _lib.host_lib()
    lp = _np_ptr(np.ascontiguousarray(lens, dtype=np.uint32), u32p) if lens is not None else None
    return int(L.kmp_synth_count_planted(lp, fixed_len, first_pkt_id, n, C.byref(sp)))


def write_udp_pcap(path: str, arena: np.ndarray, off: np.ndarray, ln: np.ndarray) -> None:
    L = _lib.host_lib()
    rc = L.kmp_write_udp_pcap(path.encode(), _np_ptr(arena, u8p), _np_ptr(off, u64p), _np_ptr(ln, u32p), len(ln))
    if rc:
        raise KmpHostError(f"kmp_write_udp_pcap failed: {rc}")


def write_udp_pcap_part(path: str, append: bool, arena: np.ndarray, off: np.ndarray, ln: np.ndarray, first_record: int = 0) -> None:
    """One part of a capture written arena by arena (kmp_write_udp_pcap_part): append=False starts the file."""
    L = _lib.host_lib()
    rc = L.kmp_write_udp_pcap_part(path.encode(), 1 if append else 0, _np_ptr(arena, u8p), _np_ptr(off, u64p), _np_ptr(ln, u32p), len(ln),
                                   first_record)
    if rc:
        raise KmpHostError(f"kmp_write_udp_pcap_part failed: {rc}")


def format_report(patterns: Sequence[bytes], counts: Sequence[int]) -> str:
    """stdout of the reference minus the elapsed line (serial.c:163-166)."""
    lines = ["Printing the number of appereances of each string throughout the entire pcap file:"]
    for p, c in zip(patterns, counts):
        if int(c) != 0:
            lines.append(f"{p.decode(errors='replace')}: {int(c)} times!")
    return "\n".join(lines) + "\n"
