"""The host code kmpgpu_load_streams_ordered adds: kmp_extract_tcp_seq, kmp_arena_from_pcap_seq (csrc/host/kmphost.c) and the parser of
KMPGPU_FLOW_STREAMS_ORDER's value (csrc/host/kmp_cli_streams_order.h), as a stand-alone program under AddressSanitizer + UBSan
(tests/streams_seq_sanitizer_driver.c), and HostArena.from_pcap(with_seq=True) over a small TCP capture written here.  No GPU needed."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import header_model as HM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.host import HostArena

A, B = 0x0A000001, 0xC0A80101


def _tcp_frame(payload, seq, sport=40000, dport=80, ihl=5, tcp_words=5):
    f = bytearray(HM.make_frame("tcp", payload, A, B, sport, dport, ihl=ihl, tcp_words=tcp_words))
    t = 14 + 4 * ihl
    f[t + 4:t + 8] = struct.pack(">I", seq)
    return bytes(f)


def _capture(path):
    """a TCP capture: in order, reordered, a retransmission, sequence numbers across 2^32, longer IP and TCP headers, one frame the tcp
    extractor rejects (cut inside its TCP header) and one UDP frame, which tcp mode reads like any other (nothing tests byte 23)"""
    rows = [(b"GET /", 1000, 5, 5), (b"in HTTP", 1008, 5, 5), (b"adm", 1005, 6, 5), (b"adm", 1005, 5, 8), (b"", 0xFFFFFFFF, 5, 5),
            (b"wrap", 0xFFFFFFFE, 15, 15), (b"x" * 300, 0x80000000, 5, 5)]
    frames = [_tcp_frame(p, s, ihl=i, tcp_words=w) for p, s, i, w in rows]
    cut = _tcp_frame(b"never", 77)
    udp = HM.make_frame("udp", b"dataPgram, long enough", A, B, 5353, 53)       # (its byte 46, 'P', reads as a 20-byte TCP header)
    records = [(len(f), f) for f in frames[:3]] + [(14 + 20 + 12, cut)] + [(len(f), f) for f in frames[3:]] + [(len(udp), udp)]
    HM.write_pcap(path, records)
    want = [(s, p) for p, s, _, _ in rows]
    t = 14 + 20
    want.append((struct.unpack(">I", udp[t + 4:t + 8])[0], None))        # the UDP frame in tcp mode: its length and checksum
    return want


def test_sanitizer_driver(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "streams_seq_driver")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-fopenmp", "-I" + os.path.join(root, "include"),
           "-I" + os.path.join(root, "multithreading_string_matching_amd", "csrc", "host"),
           os.path.join(root, "tests", "streams_seq_sanitizer_driver.c"),
           os.path.join(root, "multithreading_string_matching_amd", "csrc", "host", "kmphost.c"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    pcap = str(tmp_path / "tcp_seq.pcap")
    want = _capture(pcap)
    r = subprocess.run([exe, pcap, "tcp"], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "streams seq driver ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == f"seq {len(want)}"
    got = [tuple(int(x) for x in line.split()) for line in lines[1:1 + len(want)]]
    assert [g[0] for g in got] == [s for s, _ in want]
    assert [g[2] for g in got[:-1]] == [len(p) for _, p in want[:-1]] and [g[1] for g in got] == [6] * (len(want) - 1) + [17]


def test_extract_tcp_seq_follows_the_extractors():
    L = _lib.host_lib()
    tcp, udp = _tcp_frame(b"payload", 0xCAFEF00D, ihl=7, tcp_words=6), HM.make_frame("udp", b"payload", A, B, 1, 2)
    for frame, proto, extract in ((tcp, 1, L.kmp_extract_tcp), (udp, 0, L.kmp_extract_udp), (tcp, 0, L.kmp_extract_udp), (udp, 1, L.kmp_extract_tcp)):
        t = 14 + 4 * (frame[14] & 15)
        for cl in range(len(frame) + 1):
            buf = (C.c_uint8 * max(cl, 1)).from_buffer_copy(frame[:cl] or b"\0")
            o, l, seq = C.c_uint32(), C.c_uint32(), C.c_uint32(0xDEADBEEF)
            ok = extract(buf, cl, C.byref(o), C.byref(l))
            assert L.kmp_extract_tcp_seq(buf, cl, proto, C.byref(seq)) == ok
            assert seq.value == (struct.unpack(">I", frame[t + 4:t + 8])[0] if ok else 0xDEADBEEF)
            assert not ok or t + 8 <= cl


def test_from_pcap_with_seq(tmp_path):
    pcap = str(tmp_path / "tcp_seq.pcap")
    want = _capture(pcap)
    plain = HostArena.from_pcap(pcap, "tcp", with_meta=True)
    both = HostArena.from_pcap(pcap, "tcp", with_meta=True, with_seq=True)
    only = HostArena.from_pcap(pcap, "tcp", with_seq=True)
    assert plain.seq is None and only.meta is None
    assert both.seq.dtype == np.uint32 and both.seq.tolist() == only.seq.tolist() == [s for s, _ in want]
    for a in (both, only):                                      # the identical arena
        assert a.n_pkts == plain.n_pkts == len(want) and a.n_frames == plain.n_frames == len(want) + 1
        assert a.off.tolist() == plain.off.tolist() and a.len.tolist() == plain.len.tolist()
        assert bytes(a.bytes[:int(a.off[-1]) + 16]) == bytes(plain.bytes[:int(plain.off[-1]) + 16])
    assert both.meta.tobytes() == plain.meta.tobytes()
    off, ln = both.off, both.len
    assert [bytes(both.bytes[int(o):int(o) + int(n)]) for o, n in zip(off[:-1], ln[:-1])] == [p for _, p in want[:-1]]
    # udp mode: the one UDP frame, and the word behind its ports
    u = HostArena.from_pcap(pcap, "udp", with_seq=True)
    assert u.n_pkts >= 1 and want[-1][0] in u.seq.tolist()
    empty = str(tmp_path / "empty.pcap")
    HM.write_pcap(empty, [])
    e = HostArena.from_pcap(empty, "tcp", with_meta=True, with_seq=True)
    assert e.n_pkts == 0 and e.seq.size == 0 and e.meta.size == 0
