"""The expectations of tests/test_gpu_high_destinations.py against the plain models, on inputs small enough to build everything in full:
three periods and a rest, seven flows.  No GPU: the helper that lays the source out on the device runs with torch on the CPU.

  gpu_support.periodic_source                       decode_model.packed_image of the same payload list
  selection (index arithmetic over the period)      prep_model.gather_slots over the source's image
  decoded (test_gpu_decode_scale.expectation)       decode_model.load_decoded of the whole list
  stream_tag_counts (closed form), streams_bytes    stream_model.records, payloads and arena, the tags counted in the streams' bytes
"""
import numpy as np
import pytest

from gpu_support import PERIOD, check_periodic_bytes, period_image, periodic_bytes, periodic_end, periodic_source

import decode_model as DM
import prep_model as PM
import stream_model as TM
import test_gpu_high_destinations as HD

N = 3 * PERIOD + HD.REST
PERIODS = {"select": lambda: HD.select_period()[0], "uniform": lambda: HD.uniform_period()[0], "decode": HD.decode_base,
           "streams": HD.stream_period, "long": lambda: HD.stream_period(alternate=False)}


def listed(pay, n):
    return [pay[k % PERIOD] for k in range(n)]


def scan_counts(payloads):
    """what a scan for the tags counts: the occurrences in front of every payload's first 0x00"""
    return [sum(t.split(b"\0")[0].count(tag) for t in payloads) for tag in HD.TAGS]


@pytest.mark.parametrize("kind", sorted(PERIODS))
@pytest.mark.parametrize("n", [N, PERIOD, HD.REST, 2 * PERIOD + 1])
def test_the_device_layout_is_the_packed_image(kind, n):
    pay = PERIODS[kind]()
    tagged = [t for t in pay if len(t) >= 8]
    assert len(pay) == PERIOD and len(set(tagged)) == len(tagged) and all(t.startswith(PM.tag(e)) for e, t in enumerate(pay) if len(t) >= 8)
    arena, off, ln = DM.packed_image(listed(pay, n))
    d_arena, d_off, d_len = periodic_source(pay, n, device="cpu")
    assert d_off.dtype.is_signed and d_off.element_size() == 8 and d_len.element_size() == 4
    assert np.array_equal(d_off.numpy(), off.astype(np.int64)) and np.array_equal(d_len.numpy(), ln.astype(np.int32))
    assert periodic_end(period_image(pay), n) == len(arena) == len(d_arena) - 64
    assert np.array_equal(d_arena.numpy()[:len(arena)], arena) and not d_arena.numpy()[len(arena):].any()
    # a shorter prefix of the same tensors is the periodic arena of fewer payloads
    m = n - 57
    assert periodic_end(period_image(pay), m) == int(off[m - 1] + PM.slot_bytes(ln[m - 1:m])[0])


def check_image(want, arena, off, ln):
    assert np.array_equal(want["off"], off) and np.array_equal(want["len"], ln) and want["end"] == len(arena)
    assert np.array_equal(periodic_bytes(want), arena)
    check_periodic_bytes(np.concatenate([arena, np.zeros(64, np.uint8)]), want, rows=2)


@pytest.mark.parametrize("kind", ["select", "uniform"])
def test_selection(kind):
    pay, psel = HD.select_period() if kind == "select" else HD.uniform_period()
    for n in (N, PERIOD + 1, 2 * PERIOD):
        want = HD.selection(pay, psel, n)
        src, off, ln = DM.packed_image(listed(pay, n))
        idx = np.flatnonzero(want["sel"])
        assert np.array_equal(want["index"], idx) and want["sel"].shape == (n,)
        new_off, arena = PM.gather_slots(src, off[idx], ln[idx])
        check_image(want, arena, new_off, ln[idx])
        assert want["tags"].tolist() == scan_counts([pay[k % PERIOD] for k in idx])
    assert int(psel.sum()) < PERIOD or kind == "uniform"


def test_a_wrong_byte_is_found():
    pay, psel = HD.select_period()
    want = HD.selection(pay, psel, N)
    a = np.concatenate([periodic_bytes(want), np.zeros(64, np.uint8)])
    for at in (0, len(want["per"]) + 5, 3 * len(want["per"]) + 1, want["end"] - 1, want["end"], want["end"] + 63):
        b = a.copy()
        b[at] ^= 1
        with pytest.raises(AssertionError):
            check_periodic_bytes(b, want, rows=2)


@pytest.mark.parametrize("plus, only_changed", [(False, False), (True, True), (True, False), (False, True)])
def test_decoded(plus, only_changed):
    base = HD.decode_base()
    for n in (N, PERIOD + 1):
        want = HD.decoded(base, n, plus, only_changed)
        m = DM.load_decoded(listed(base, n), plus, only_changed)
        check_image(want, m["arena"], m["off"], m["len"])
        assert np.array_equal(want["index"], m["index"]) and np.array_equal(want["changed"], m["changed"]) and want["stats"] == m["stats"]
        assert want["tags"].tolist() == scan_counts(m["payloads"])
        full = HD.expectation(base, n, plus, only_changed)                # the scale module's own tiling
        assert np.array_equal(full["arena"], m["arena"]) and np.array_equal(full["index"], m["index"]) and full["stats"] == m["stats"]


def test_decode_period_takes_both_write_paths():
    base = HD.decode_base()
    straight, staged = HD.write_paths(base)
    assert all(not DM.changed(base[e], True) for e in straight) and all(DM.changed(base[e]) for e in staged)
    assert len(straight) > PERIOD // 4 and len(staged) > PERIOD // 4
    assert HD.write_paths([b"abc%41" + b"x" * 26, b"%41" + b"x" * 13 + b"%42", b"x" * 16 + b"%41" + b"x" * 13 + b"%42"]) == ([], [1, 2])
    assert all(t.startswith(PM.tag(e)) for e, t in enumerate(base))


@pytest.mark.parametrize("alternate", [True, False])
def test_streams(alternate):
    pay = HD.stream_period(alternate)
    image = period_image(pay)
    meta = HD.flows_of(N, n_flows=7)
    lens = HD.period_lens(pay, N)
    src = listed(pay, N)
    assert lens.tolist() == [len(t) for t in src]
    uncut, _ = TM.records(meta, lens, 1 << 30)
    cut = (int(uncut["bytes"][uncut["dir"] == 0].min()) - 1) // 16 * 16
    for depth in (1 << 30, cut, cut - 7, cut - 15, 1458, 8, 7):
        recs, pos = TM.records_np(meta, lens, depth)
        slow = TM.records(meta, lens, depth)
        assert recs.tobytes() == slow[0].tobytes() and pos.tobytes() == slow[1].tobytes() and len(recs) == 14
        assert HD.cut_to(uncut, depth).tobytes() == recs.tobytes()
        assert (recs["bytes"][recs["dir"] == 0] > recs["bytes"][recs["dir"] == 1]).all()      # direction 0 is the forward one
        streams = TM.payloads(src, meta, depth)
        arena, off, ln = TM.arena(streams)
        soff, size = HD.stream_index(recs)
        assert np.array_equal(soff.astype(np.uint64), off) and np.array_equal(recs["len"], ln) and int(size.sum()) == len(arena)
        assert HD.stream_tag_counts(recs, pos).tolist() == scan_counts(streams)
        for chosen in (np.arange(len(recs)), np.array([0, 3, len(recs) - 1]), np.array([5])):
            want, woff = HD.streams_bytes(image, lens, recs, pos, chosen)
            for j, s in enumerate(chosen.tolist()):
                assert np.array_equal(want[woff[j]:woff[j] + size[s]], arena[soff[s]:soff[s] + size[s]]), (depth, s)


def test_chosen_streams():
    soff = np.arange(10_000, dtype=np.int64) * (1 << 20)
    s32, chosen = HD.chosen_streams(soff, len(soff))
    assert s32 == 4096 and {0, 1, 2, 3, 4094, 4095, 4096, 4097, 4098, 9996, 9997, 9998, 9999} <= set(chosen.tolist())
    assert 64 <= len(chosen) <= 77 and (np.diff(chosen) > 0).all()
