"""What the nine calls that build dst's arena out of src's on the GPU have in common, on a real MI355X: kmpgpu_load_selected, _decoded,
_base64, _fields, _dns, _tls, _seams, _streams and _streams_ordered refuse the same wrong pairs of contexts with the same codes, leave the
other context's arena alone when they do, empty dst for a src without payloads, and report the launch counts of include/kmpgpu.h.

src holds three payloads of one flow direction with metadata and built flows, so that every one of the calls is legal on it; dst has no
patterns and holds two other payloads.  What each call computes is the matter of its own module (tests/test_gpu_select.py, _decode, _base64,
_fields, _dns, _tls, _seams, _streams, _streams_seq).

No test provokes a fault: every refusal is a check on the host that returns before anything is launched.

Run on a real MI355X:  python -m pytest tests/test_gpu_derived_contract.py -m gpu
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import EMPTY_ARENA, load, reset  # noqa: E402  (torch first)

from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.host import META_DTYPE  # noqa: E402
from multithreading_string_matching_amd.matcher import DECODE_PERCENT, DNS_QNAME, FIELD_RAW_URI, TLS_SNI, GpuMatcher, device_count  # noqa: E402

OK, EINVAL, ESTATE = 0, -2, -3
PAYLOADS = [b"GET /a%20b?x=aGVsbG8gd29ybGQsIGhlbGxv HTTP/1.1\r\nHost: one\r\n\r\n", b"POST /c%41 HTTP/1.1\r\nHost: two\r\n\r\nbody", b"tail of it"]
KEPT = [b"kept", b"these two"]
KEPT_INFO = (2, sum(len(p) for p in KEPT))
SRC_INFO = (3, sum(len(p) for p in PAYLOADS))

WORDS = np.full(8, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)        # kmpgpu_load_selected: every payload; the others: where the bitmap goes
SEQ = (1000 + np.concatenate([[0], np.cumsum([len(p) for p in PAYLOADS])[:-1]])).astype(np.uint32)

# name -> (the call with valid arguments on (dst, src), launches of a successful call on the three payloads, launches of a second one)
#   selected: phase 1's three, the copy, the index check's one, and the metadata's move           kmpgpu.h, kmpgpu_load_selected
#   decoded, base64: lengths, two scan kernels, index, write                                       kmpgpu.h, kmpgpu_load_decoded
#   fields, dns, tls: the same five and the locate where src's spans are stale                     kmpgpu.h, kmpgpu_load_fields
#   seams: keys, sort, phase 1's three, index, gather                                              kmpgpu.h, kmpgpu_load_seams
#   streams: 10, ordered streams: 16                                                               kmpgpu.h, kmpgpu_load_streams(_ordered)
CALLS = {
    "selected": (lambda g, d, s: g.kmpgpu_load_selected(d, s, WORDS.ctypes.data, 0, None), 6, 6),
    "decoded": (lambda g, d, s: g.kmpgpu_load_decoded(d, s, DECODE_PERCENT, 0, WORDS.ctypes.data, None, None), 5, 5),
    "base64": (lambda g, d, s: g.kmpgpu_load_base64(d, s, 16, 0, WORDS.ctypes.data, None, None), 5, 5),
    "fields": (lambda g, d, s: g.kmpgpu_load_fields(d, s, FIELD_RAW_URI, 0, WORDS.ctypes.data, None, None), 6, 5),
    "dns": (lambda g, d, s: g.kmpgpu_load_dns(d, s, DNS_QNAME, 0, WORDS.ctypes.data, None, None), 6, 5),
    "tls": (lambda g, d, s: g.kmpgpu_load_tls(d, s, TLS_SNI, 0, WORDS.ctypes.data, None, None), 6, 5),
    "seams": (lambda g, d, s: g.kmpgpu_load_seams(d, s, 16, None), 7, 7),
    "streams": (lambda g, d, s: g.kmpgpu_load_streams(d, s, 1 << 20, None), 10, 10),
    "streams_ordered": (lambda g, d, s: g.kmpgpu_load_streams_ordered(d, s, 1 << 20, SEQ.ctypes.data, 0, None), 16, 16),
}
NAMES = list(CALLS)


@pytest.fixture(scope="module")
def contexts():
    src, dst = GpuMatcher(0), GpuMatcher(0)
    src.set_patterns([b"x"])
    yield src, dst
    src.close()
    dst.close()


@pytest.fixture
def pair(contexts):
    """(g, src, dst): src with the three payloads, their metadata and flows, and no spans yet; dst with its own two"""
    src, dst = contexts
    reset(src, dst)
    WORDS[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    load(src, PAYLOADS)
    meta = np.zeros(len(PAYLOADS), dtype=META_DTYPE)
    meta["src_ip"], meta["dst_ip"], meta["src_port"], meta["dst_port"], meta["proto"] = 0x0A000001, 0xC0A80101, 40001, 80, 6
    src.set_meta(meta)
    assert src.build_flows() == 1
    load(dst, KEPT)
    assert src.arena_info() == SRC_INFO and dst.arena_info() == KEPT_INFO
    return _lib.gpu_lib(), src, dst


@pytest.fixture(scope="module")
def frames():
    fr = _lib.Frames()
    err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
    assert _lib.host_lib().kmp_frames_from_pcap(os.path.join(DATA, "udp_1000.pcap").encode(), None, None, C.byref(fr), err) == 0
    yield fr
    _lib.host_lib().kmp_frames_free(C.byref(fr))


@pytest.mark.parametrize("name", NAMES)
def test_null_and_same_context(pair, name):
    g, src, dst = pair
    call = CALLS[name][0]
    for d, s, what in ((None, src._ctx, b"ctx is NULL"), (dst._ctx, None, b"ctx is NULL"), (dst._ctx, dst._ctx, b"same context"),
                       (src._ctx, src._ctx, b"same context")):
        assert call(g, d, s) == EINVAL
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_" + name.encode() + b":" in msg and what in msg, msg
        assert src.arena_info() == SRC_INFO and dst.arena_info() == KEPT_INFO


@pytest.mark.parametrize("name", NAMES)
def test_between_load_frames_begin_and_finish(pair, frames, name):
    g, src, dst = pair
    call = CALLS[name][0]
    fr = frames
    with GpuMatcher(0) as other:
        other.set_patterns([b"ab"])
        assert g.kmpgpu_load_frames_begin(other._ctx, fr.bytes, fr.nbytes, fr.off, fr.caplen, fr.n, 0) == 0
        try:
            assert call(g, other._ctx, src._ctx) == ESTATE
            msg = g.kmpgpu_last_error()
            assert b"kmpgpu_load_" + name.encode() + b":" in msg and b"dst sits between" in msg, msg
            assert src.arena_info() == SRC_INFO
            assert call(g, dst._ctx, other._ctx) == ESTATE
            msg = g.kmpgpu_last_error()
            assert b"kmpgpu_load_" + name.encode() + b":" in msg and b"src sits between" in msg, msg
            assert dst.arena_info() == KEPT_INFO
        finally:
            n = C.c_uint64()
            assert g.kmpgpu_load_frames_finish(other._ctx, C.byref(n)) == 0


@pytest.mark.parametrize("name", NAMES)
def test_src_without_payloads(pair, name):
    g, src, dst = pair
    src.load_arena(*EMPTY_ARENA)
    assert src.build_flows() == 0                      # (seams and streams ask for built flows, of no payloads too)
    assert CALLS[name][0](g, dst._ctx, src._ctx) == OK, g.kmpgpu_last_error()
    assert dst.arena_info() == (0, 0)
    assert dst.last_timing().launches == 0


@pytest.mark.parametrize("name", NAMES)
def test_launches(pair, name):
    g, src, dst = pair
    call, first, again = CALLS[name]
    assert call(g, dst._ctx, src._ctx) == OK, g.kmpgpu_last_error()
    assert dst.last_timing().launches == first
    assert dst.arena_info()[0] == {"seams": 2, "streams": 1, "streams_ordered": 1}.get(name, 3)
    assert call(g, dst._ctx, src._ctx) == OK, g.kmpgpu_last_error()
    assert dst.last_timing().launches == again
    assert src.arena_info() == SRC_INFO


@pytest.mark.parametrize("name", NAMES)
def test_two_devices(pair, name):
    g, src, dst = pair
    if device_count() < 2:
        pytest.skip("one device: no two contexts on two devices")
    with GpuMatcher(1) as far:
        assert CALLS[name][0](g, far._ctx, src._ctx) == EINVAL
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_" + name.encode() + b":" in msg and b"the contexts sit on devices" in msg, msg
        assert src.arena_info() == SRC_INFO
