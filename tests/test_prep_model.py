"""The numpy model of the arena-building kernels (tests/prep_model.py) against the host library and the CPU oracle.

tests/test_gpu_prep_scale.py compares kmpgpu_load_frames, the repack and the padding pass with this model at millions of
entries; here the model itself is held to ``HostArena.from_pcap`` (serial.c:115-141 restated in C, itself held to the reference's
object code by tests/test_oracle.py) on the same frames written out as a capture file, byte for byte.  No GPU needed.
"""
import numpy as np
import pytest

import multithreading_string_matching_amd as K
import prep_model as PM


@pytest.fixture(scope="module")
def frames():
    return PM.frame_library()


def test_library_covers_what_it_promises(frames, oracle):
    assert 300 <= len(frames) <= 1000 and sum(map(len, frames)) < 200_000
    for proto in ("udp", "tcp"):
        poff, plen = PM.library_rule(frames, proto, oracle.dump)
        lens = set(plen.tolist())
        assert PM.REJECTED in lens and (plen < 0).sum() >= 50
        for L in PM.PAYLOAD_LENGTHS + PM.BIG_LENGTHS:
            assert L in lens, (proto, L)
        assert (plen == 1458).sum() >= 2 and (plen == 0).sum() >= 2
        pay = PM.library_payloads(frames, poff, plen)
        own = PM.own_tag_kinds(pay)
        assert len(own) >= 60 and all(plen[t] >= 8 for t in own)
        assert any(p is not None and b"\0" in p for p in pay)                  # effective bytes differ from payload bytes


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_rule_equals_the_host_library_per_frame(frames, oracle, proto):
    poff, plen = PM.library_rule(frames, proto, oracle.dump)
    for k, f in enumerate(frames):
        r = K.extract(f, len(f), proto)
        assert (r is None) == (plen[k] < 0), k
        if r is not None:
            assert r == (int(poff[k]), int(plen[k])), k


@pytest.mark.parametrize("proto", ["udp", "tcp"])
@pytest.mark.parametrize("shape,n", [("mixed", 120_000), ("rejected_stretch", 100_000), ("all_empty", 5_000), ("last_only", 3_000), ("all_rejected", 2_000)])
def test_model_equals_host_arena_from_pcap(frames, oracle, tmp_path, proto, shape, n):
    poff, plen = PM.library_rule(frames, proto, oracle.dump)
    blob, boff, _ = PM.library_blob(frames)
    if shape == "rejected_stretch":                     # longer than one 1024-item tile of the device scan, mixed kinds around it
        kind = PM.make_sequence("mixed", n, plen, 5)
        rej = np.flatnonzero(plen < 0)
        kind[40_000:43_000] = rej[np.arange(3_000) % len(rej)]
    else:
        kind = PM.make_sequence(shape, n, plen, 5)
    path = tmp_path / "lib.pcap"
    PM.write_pcap(str(path), frames, kind)
    host = K.HostArena.from_pcap(str(path), proto)
    acc, off, ln, arena = PM.extraction_arena(blob, boff, poff, plen, kind)
    assert host.n_frames == n and host.n_pkts == len(acc) == int((plen[kind] >= 0).sum())
    assert host.payload_bytes == int(ln.sum(dtype=np.uint64))
    assert np.array_equal(host.len, ln) and np.array_equal(host.off, off)
    assert np.array_equal(host.bytes[:len(arena)], arena)                       # payload bytes AND zero padding
    if len(acc):
        acc2, off2, ln2, _ = PM.extraction_index(boff, poff, plen, kind)
        assert np.array_equal(acc2, acc) and np.array_equal(off2, off) and np.array_equal(ln2, ln)
        assert PM.effective_bytes(arena, off, ln) == sum((p.find(b"\0") + 1) or len(p) for p in (host.payload(k) for k in range(0, host.n_pkts)))
        # tags: what a scan has to count, from the model alone, equals the oracle's count over the host library's arena
        pay = PM.library_payloads(frames, poff, plen)
        want = PM.tag_counts(pay, acc, len(frames))
        tags = [PM.tag(t) for t in range(len(frames))]
        got, _ = oracle.count(host.bytes, host.off, host.len, tags, threads=4)
        assert got.tolist() == want.tolist()
        own = PM.own_tag_kinds(pay)
        assert want[own].tolist() == np.bincount(acc, minlength=len(frames))[own].tolist()


def test_repack_and_padding_models(oracle):
    arena, off, ln = PM.shuffled_arena(30_000, 3)
    slot = PM.slot_bytes(ln)
    order = np.argsort(off)
    assert np.all(off % 16 == 0) and np.all(off[order][1:] >= (off + slot)[order][:-1]) and int((off + slot).max()) + 64 == len(arena)
    assert not np.array_equal(order, np.arange(len(off))) and (arena == 0).sum() > 0
    payloads = [arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(off, ln)]
    host = K.HostArena.from_payloads(payloads)
    new_off, packed = PM.gather_slots(arena, off, ln)
    assert np.array_equal(new_off, host.off) and np.array_equal(packed, host.bytes[:len(packed)])
    assert PM.effective_bytes(arena, off, ln) == PM.effective_bytes(packed, new_off, ln) == sum((p.find(b"\0") + 1) or len(p) for p in payloads)
    clean = PM.clean_padding(arena, off, ln)
    ref = arena.copy()
    for o, l, s in zip(off.tolist(), ln.tolist(), slot.tolist()):
        ref[o + l:o + s] = 0
    assert np.array_equal(clean, ref) and not np.array_equal(clean, arena)
    pats = [b"ab", b"abcab", b"b"]
    assert oracle.count(clean, off, ln, pats)[0].tolist() == oracle.count(packed, new_off, ln, pats)[0].tolist()
