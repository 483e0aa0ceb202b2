"""The host side of kmpgpu_load_selected (no GPU needed): how GpuMatcher.load_selected packs its argument and maps the selection
back to the source, the multi-part capture writer the command lines export through, and their refusal of an export path that
cannot be written -- with exit code 1, where a run that got as far as looking for a GPU would end with 2 on a machine without one.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA

import multithreading_string_matching_amd as K
from multithreading_string_matching_amd import _lib, host
from multithreading_string_matching_amd.matcher import select_words, selected_indices

SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 1000]


def _model_words(sel):
    """bit k & 63 of word k >> 6, by hand"""
    W = (len(sel) + 63) // 64
    words = [0] * W
    for k, s in enumerate(sel):
        if s:
            words[k >> 6] |= 1 << (k & 63)
    return words


@pytest.mark.parametrize("n", SIZES)
def test_bool_selection_is_packed_lsb_first(n):
    rng = np.random.default_rng(n)
    cases = [np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 2 == 0, np.arange(n) % 2 == 1, rng.random(n) < 0.1, rng.random(n) < 0.9]
    if n:
        only_first = np.zeros(n, bool); only_first[0] = True
        only_last = np.zeros(n, bool); only_last[-1] = True
        cases += [only_first, only_last]
    for sel in cases:
        words = select_words(sel, n)
        assert words.dtype == np.uint64 and words.shape == ((n + 63) // 64,) and words.flags.c_contiguous
        assert [int(w) for w in words] == _model_words(sel.tolist())
        idx = selected_indices(words, n)
        assert idx.dtype == np.uint64 and idx.tolist() == np.flatnonzero(sel).tolist()


@pytest.mark.parametrize("n", SIZES)
def test_words_pass_through_and_dirty_bits_above_n_are_ignored(n):
    rng = np.random.default_rng(100 + n)
    W = (n + 63) // 64
    sel = rng.random(n) < 0.5
    words = np.array(_model_words(sel.tolist()), dtype=np.uint64).reshape(W)
    assert select_words(words, n).tolist() == words.tolist()
    dirty = words.copy()
    if n % 64:
        dirty[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1))        # every bit at n and above
        assert int(dirty[-1]) >> (n % 64) == (1 << (64 - n % 64)) - 1
    assert select_words(dirty, n).tolist() == dirty.tolist()                   # handed over as they are: the library ignores them
    assert selected_indices(dirty, n).tolist() == np.flatnonzero(sel).tolist()
    all_ones = np.full(W, np.uint64((1 << 64) - 1), dtype=np.uint64)
    assert selected_indices(all_ones, n).tolist() == list(range(n))


def test_selection_arguments_that_do_not_fit():
    with pytest.raises(ValueError):
        select_words(np.zeros(64, bool), 65)
    with pytest.raises(ValueError):
        select_words(np.zeros(2, np.uint64), 64)
    with pytest.raises(ValueError):
        select_words(np.zeros(1, np.int64), 64)
    with pytest.raises(ValueError):
        select_words(np.zeros(0, np.uint64), 1)


def _payload_arena(payloads):
    a = K.HostArena.from_payloads(payloads)
    return a


def test_capture_written_in_parts_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    lens = [0, 1, 15, 16, 17, 48, 1500, 9000, 3, 0, 700]
    payloads = [bytes(rng.integers(0, 256, L).astype(np.uint8)) for L in lens]
    whole, parts = str(tmp_path / "whole.pcap"), str(tmp_path / "parts.pcap")
    a = _payload_arena(payloads)
    host.write_udp_pcap(whole, a.bytes, a.off, a.len)
    # three arenas, the second one without payloads, into one file
    cuts = [(0, 4), (4, 4), (4, len(payloads))]
    written = 0
    host.write_udp_pcap_part(parts, False, np.zeros(16, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0)
    empty = K.HostArena.from_pcap(parts, "udp")
    assert empty.n_pkts == 0 and os.path.getsize(parts) == 24
    for lo, hi in cuts:
        if hi > lo:
            p = _payload_arena(payloads[lo:hi])
            host.write_udp_pcap_part(parts, True, p.bytes, p.off, p.len, written)
        else:
            host.write_udp_pcap_part(parts, True, np.zeros(16, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), written)
        written += hi - lo
    with open(whole, "rb") as f, open(parts, "rb") as g:
        assert f.read() == g.read()
    back = K.HostArena.from_pcap(parts, "udp")
    assert back.n_pkts == len(payloads)
    assert [back.payload(k) for k in range(back.n_pkts)] == payloads
    # append == 0 starts over
    p = _payload_arena(payloads[:2])
    host.write_udp_pcap_part(parts, False, p.bytes, p.off, p.len, 0)
    back = K.HostArena.from_pcap(parts, "udp")
    assert [back.payload(k) for k in range(back.n_pkts)] == payloads[:2]
    with pytest.raises(host.KmpHostError):
        host.write_udp_pcap_part(str(tmp_path / "no_such_dir" / "x.pcap"), False, p.bytes, p.off, p.len, 0)


@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["2"])])
def test_cli_refuses_an_export_path_it_cannot_write(tmp_path, prog, extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("KMPGPU_")}
    env["KMPGPU_EXPORT_FILE"] = str(tmp_path / "no_such_dir" / "out.pcap")
    r = subprocess.run([os.path.join(_lib.BINDIR, prog), os.path.join(DATA, "udp_1000.pcap"), os.path.join(DATA, "strings.txt"), *extra, "udp"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "KMPGPU_EXPORT_FILE" in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    # a windows file counts the export as the output it acts on: the refusal is the path's, not the windows'
    wf = tmp_path / "windows.txt"
    wf.write_text("0 0 0\n")
    env["KMPGPU_WINDOWS_FILE"] = str(wf)
    r = subprocess.run([os.path.join(_lib.BINDIR, prog), os.path.join(DATA, "udp_1000.pcap"), os.path.join(DATA, "strings.txt"), *extra, "udp"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "KMPGPU_EXPORT_FILE" in r.stderr and "no effect" not in r.stderr and r.stdout == ""
    # ... and so do rules without an alerts file
    rf = tmp_path / "rules.txt"
    rf.write_text("0\n")
    env["KMPGPU_RULES_FILE"] = str(rf)
    r = subprocess.run([os.path.join(_lib.BINDIR, prog), os.path.join(DATA, "udp_1000.pcap"), os.path.join(DATA, "strings.txt"), *extra, "udp"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 1 and "KMPGPU_EXPORT_FILE" in r.stderr and "go together" not in r.stderr and r.stdout == ""
