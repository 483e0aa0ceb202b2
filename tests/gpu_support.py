"""What the GPU test modules share: the context fixture, the options' defaults, the kernel selections, borrowed arenas with dirty
padding, the command lines, and the exact comparisons of a pass's outputs with tests/match_model.py's answers.

Import from this module before the package, for the reason given below.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA

# torch first: its wheel carries its own ROCm runtime libraries, and a process in which the system's libamdhip64 (what libkmpgpu.so
# links) is loaded BEFORE torch's ends up with torch seeing "No HIP GPUs" (seen when a GPU test file was run on its own; in the whole
# suite tests/test_dist.py imports torch earlier).  The C-ABI library itself does not care which of the two it gets.
import torch  # noqa: E402

import match_model as MM  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.host import HostArena  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, KERNEL_FLAT, KERNEL_GENERAL, KERNEL_PACKED, MODE_AUTOMATON, MODE_FILTER, OPT_ACCUMULATE, OPT_BLOCKS_PER_CU, OPT_DEPTH,
    OPT_FUSED, OPT_FUSED_UNIT, OPT_KERNEL, OPT_MODE, OPT_NONTEMPORAL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher)

# (name, kernel, fused): the automatic choice (fused for multi-pattern sets) and the two streaming kernels on their own
KERNELS = [("auto", KERNEL_AUTO, 2), ("flat", KERNEL_FLAT, 0), ("packed", KERNEL_PACKED, 0)]
# (name, mode, kernel, fused): every kernel family
VARIANTS = [("auto", MODE_FILTER, KERNEL_AUTO, 2), ("flat", MODE_FILTER, KERNEL_FLAT, 0), ("packed", MODE_FILTER, KERNEL_PACKED, 0),
            ("general", MODE_FILTER, KERNEL_GENERAL, 0), ("automaton", MODE_AUTOMATON, KERNEL_GENERAL, 0), ("fused", MODE_FILTER, KERNEL_AUTO, 1)]

# every option a test of the suite changes, and its default.  kmpgpu_set_option only stores the value in the context: writing a
# default over a default invalidates no plan and no buffer, so every module restores all of them.
DEFAULTS = ((OPT_MODE, MODE_FILTER), (OPT_KERNEL, KERNEL_AUTO), (OPT_FUSED, 2), (OPT_REPACK, 1), (OPT_ACCUMULATE, 0), (OPT_WHOLE_PAYLOAD, 0),
            (OPT_FUSED_UNIT, 0), (OPT_DEPTH, 0), (OPT_BLOCKS_PER_CU, 0), (OPT_NONTEMPORAL, 1))


@pytest.fixture(scope="module")
def gm():
    """one context per test module that imports this fixture"""
    m = GpuMatcher(0)
    yield m
    m.close()


def reset(*ms):
    for m in ms:
        for key, value in DEFAULTS:
            m.set_option(key, value)


# ------------------------------------------------------------------------------------------------
# arenas
# ------------------------------------------------------------------------------------------------
def attach_slots(gm, payloads, slots):
    """a borrowed arena (attach_arena) keeps what lies in its padding: slots[k] = payload k and the bytes behind it up to its slot's end;
    the kernels take each payload's end from the index.  Returns the device tensors, which the caller keeps alive."""
    ln = np.array([len(t) for t in payloads], dtype=np.uint32)
    size = np.array([len(s) for s in slots], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64)
    arena = np.frombuffer(b"".join(slots) + b"\0" * 64, dtype=np.uint8).copy()
    keep = (torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    gm.attach_arena(*keep)
    return keep


def load(gm, payloads, slots=None):
    """the payloads as an arena of the library's own, or, with slots, as attach_slots"""
    if slots is None:
        gm.load_arena(HostArena.from_payloads(payloads))
        return None
    return attach_slots(gm, payloads, slots)


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
def strip_elapsed(out):
    lines = out.splitlines(keepends=True)
    assert lines and lines[-1].startswith("Elapsed time = ") and lines[-1].endswith(" seconds\n")
    return "".join(lines[:-1])


def run_cli(prog, pcap="udp_1000.pcap", strings="strings.txt", extra=(), env_extra=None, mode="udp", scrub="KMPGPU_"):
    """prog <pcap> <strings> [extra ...] [mode], the two files from tests/golden/data unless given as absolute paths.  The caller's
    environment variables that start with `scrub` are not passed on (None: all of them are); env_extra is added."""
    env = {k: v for k, v in os.environ.items() if not (scrub and k.startswith(scrub))}
    env.update(env_extra or {})
    return subprocess.run([os.path.join(_lib.BINDIR, prog), os.path.join(DATA, pcap), os.path.join(DATA, strings), *extra, *([mode] if mode else [])],
                          capture_output=True, text=True, timeout=300, env=env)


# ------------------------------------------------------------------------------------------------
# one pass against the model, exactly
# ------------------------------------------------------------------------------------------------
def check_offsets(gm, recs, counts):
    got, found, cnt = gm.scan_offsets(max(sum(counts), 1))
    assert found == len(recs)
    assert cnt.tolist() == list(counts)
    got = MM.triples(got)
    assert len(got) == len(set(got))                  # no record twice
    want = sorted(recs)
    assert got == want, ([x for x in got if x not in recs][:6], [x for x in want if x not in set(got)][:6])


def check_packets(gm, hits, counts):
    res = gm.scan_packets(hits=True)
    bad = np.argwhere(res["hits"] != hits)
    assert bad.size == 0, [(int(i), int(k), bool(hits[i, k])) for i, k in bad[:8]]
    assert res["pkt_counts"].tolist() == hits.sum(axis=1).tolist()
    assert res["any"].tolist() == hits.any(axis=0).tolist()
    assert res["counts"].tolist() == list(counts)
    return res


def check_rules(gm, mat, rules, counts):
    """mat: the rows the rules' terms index -- the hit matrix, with the relation rows behind it where relations are set"""
    rows = MM.rule_rows(mat, rules)
    res = gm.scan_rules(hits=True)
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, [(int(r), int(k), bool(rows[r, k])) for r, k in bad[:8]]
    assert res["rule_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    assert res["counts"].tolist() == list(counts)
    return res


def check_relations(gm, rows, counts):
    res = gm.scan_relations(hits=True)
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, [(int(q), int(k), bool(rows[q, k]), gm.relations[int(q)]) for q, k in bad[:8]]
    assert res["rel_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    assert res["counts"].tolist() == list(counts)
    return res
