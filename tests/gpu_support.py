"""What the GPU test modules share: the context fixture, the options' defaults, the kernel selections, borrowed arenas with dirty
padding and arenas placed around offset 2^32 of one large buffer, periodic arenas of any size laid out on the device and what a second
arena built from one has to hold, the frame library of tests/prep_model.py and its loader, the command lines, and the exact comparisons of a pass's outputs
with the answers of tests/match_model.py and tests/flow_model.py.

Import from this module before the package, for the reason given below.
"""
import ctypes as C
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
import prep_model as PM  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.host import META_DTYPE, HostArena  # noqa: E402
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
# placed arenas: a small borrowed arena at a chosen place of one buffer of a little over 4 GiB, so that its payloads lie in front of,
# across and behind offset 2^32 (tests/test_gpu_high_offsets.py says what that is for)
# ------------------------------------------------------------------------------------------------
B32 = 1 << 32
PLACED_LOW = 4 << 20                                   # base 0: the arena lies inside [0, PLACED_LOW)
PLACED_FROM, PLACED_TO = B32 - (4 << 20), B32 + (8 << 20)      # every other base: inside [PLACED_FROM, PLACED_TO), the buffer's end
PLACEMENTS = ("low", "split", "edge", "behind")
SPLIT_FRONT = 48                                       # bytes of the straddling payload in front of 2^32 under `split`


def make_big_buffer():
    return torch.zeros(PLACED_TO, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def big_buffer():
    """one zeroed device buffer from offset 0 to 2^32 + 8 MiB per module that asks for it; the library's fold buffer of a nocase set adds
    up to 4 GiB beside it"""
    buf = make_big_buffer()
    yield buf
    del buf
    torch.cuda.empty_cache()


def zero_slots(payloads):
    """every payload followed by 0x00 up to the end of its 16-byte slot, 16 bytes for an empty payload"""
    return [t + b"\0" * ((-len(t)) % 16 or (0 if t else 16)) for t in payloads]


def slot_offsets(slots):
    """(offset of every slot from the arena's first byte as int64, end of the last slot)"""
    size = np.array([len(s) for s in slots], dtype=np.int64)
    assert (size % 16 == 0).all() and (size >= 16).all()
    end = np.cumsum(size)
    return end - size, int(end[-1])


def placed_base(placement, payloads, slots=None, k=None):
    """The arena's first byte for a placement, from the payload list.  low: 0.  split: payload k has SPLIT_FRONT bytes in front of 2^32 and
    the rest behind; k is no multiple of 64 and more than 64 payloads follow it, so the wavefront of a per-payload kernel that holds it
    has lanes on both sides.  edge: payload k starts at 2^32, the slot in front of it ends there.  behind: 2^32 + 4096 + 48 -- every
    offset is above 2^32 and the first payload is on no 128-byte line."""
    off, end = slot_offsets(zero_slots(payloads) if slots is None else slots)
    if placement == "low":
        base = 0
    elif placement == "split":
        assert k % 64 and len(payloads) - 1 - k > 64 and len(payloads[k]) > SPLIT_FRONT + 64
        base = B32 - int(off[k]) - SPLIT_FRONT
    elif placement == "edge":
        assert 0 < k < len(payloads) and payloads[k] and payloads[k - 1]
        base = B32 - int(off[k])
    else:
        assert placement == "behind"
        base = B32 + 4096 + 48
        assert base % 128
    assert base % 16 == 0
    assert base + end <= PLACED_LOW if placement == "low" else PLACED_FROM <= base and base + end + 64 <= PLACED_TO
    if placement in ("split", "edge"):
        assert base < B32 < base + end
    return base


def attach_placed(gm, payloads, slots, base, buf, off=None):
    """attach_slots at absolute offsets inside buf (the big_buffer fixture): the slots are written to buf[base : base + end), everything
    else of the two windows a placement may use is zeroed first -- a case never sees the one before it --, and the arena is attached with
    the offsets off + base and arena_bytes = base + end, the end of the last slot.  off: the slots' offsets from base where they are not
    back to back (every slot inside one of the two windows).  Returns the tensors to keep alive."""
    slots = zero_slots(payloads) if slots is None else slots
    assert base % 16 == 0 and all(s.startswith(t) for t, s in zip(payloads, slots))
    if off is None:
        off, end = slot_offsets(slots)
        spans = [(base, b"".join(slots))]
    else:
        off = np.asarray(off, dtype=np.int64)
        assert (off % 16 == 0).all()
        end = max(int(o) + len(s) for o, s in zip(off, slots))
        spans = [(base + int(o), s) for o, s in zip(off, slots)]
    for lo, data in spans:
        assert (0 <= lo and lo + len(data) <= PLACED_LOW) or (PLACED_FROM <= lo and lo + len(data) + 64 <= PLACED_TO), (lo, len(data))
    assert buf.numel() == PLACED_TO
    buf[:PLACED_LOW].zero_()
    buf[PLACED_FROM:].zero_()
    if len(spans) == 1:
        lo, data = spans[0]
        buf[lo:lo + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    else:                                              # scattered slots: one image per window, copied whole
        for w0, w1 in ((0, PLACED_LOW), (PLACED_FROM, PLACED_TO)):
            mine = [(lo, d) for lo, d in spans if w0 <= lo < w1]
            if mine:
                img = np.zeros(max(lo + len(d) for lo, d in mine) - w0, dtype=np.uint8)
                for lo, d in mine:
                    img[lo - w0:lo - w0 + len(d)] = np.frombuffer(d, dtype=np.uint8)
                buf[w0:w0 + len(img)] = torch.from_numpy(img).cuda()
    ln = np.array([len(t) for t in payloads], dtype=np.int32)
    keep = (buf, torch.from_numpy(off + base).cuda(), torch.from_numpy(ln).cuda())
    torch.cuda.synchronize()
    gm.attach_arena(*keep, arena_bytes=base + end)
    return keep


# ------------------------------------------------------------------------------------------------
# periodic arenas: payload k = period entry k % P, laid out on the device, and what a second arena built from one has to hold
# (tests/test_gpu_high_destinations.py; tests/test_high_destinations_model.py holds all of this to the plain models on the CPU)
# ------------------------------------------------------------------------------------------------
PERIOD = 257
EMPTY_ARENA = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


def tagged(body, e):
    """body with prep_model.tag(e) over its first 8 bytes; a body shorter than the tag stays as it is"""
    return PM.tag(e) + body[8:] if len(body) >= 8 else body


def period_image(payloads):
    """(bytes uint8, off int64[P], len int64[P]) of the packed image of one period: slots of max(16, round_up(len, 16)) bytes back to
    back from 0, 0x00 behind every payload's end"""
    ln = np.array([len(t) for t in payloads], dtype=np.int64)
    slot = PM.slot_bytes(ln).astype(np.int64)
    off = np.cumsum(slot) - slot
    img = np.zeros(int(slot.sum()), dtype=np.uint8)
    for o, t in zip(off.tolist(), payloads):
        img[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return img, off, ln


def periodic_end(image, n):
    """the end of the last slot of the first n payloads of the periodic arena over `image`"""
    img, off, _ = image
    reps, rest = divmod(n, len(off))
    return reps * len(img) + (int(off[rest]) if rest else 0)


def periodic_source(payloads, n, device="cuda"):
    """The packed arena with clean padding of n payloads, payload k = payloads[k % P], made by torch on `device`: the period's image
    copied into every row of the arena seen as [n // P, image bytes] (what repeat() gives, written in place), then the image's head for
    the n % P payloads that are left and 64 bytes of 0x00; offsets and lengths by arithmetic over arange(n).  Nothing of the arena's size
    exists on the host.  Returns (arena uint8, off int64[n], len int32[n]); the first m payloads are a periodic arena as well, which
    ends at periodic_end(image, m)."""
    P = len(payloads)
    img, poff, pln = period_image(payloads)
    reps, rest = divmod(n, P)
    pb, end = len(img), periodic_end((img, poff, pln), n)
    d_img = torch.from_numpy(img).to(device)
    arena = torch.zeros(end + 64, dtype=torch.uint8, device=device)
    if reps:
        arena[:reps * pb].view(reps, pb).copy_(d_img.expand(reps, pb))
    arena[reps * pb:end] = d_img[:end - reps * pb]
    k = torch.arange(n, dtype=torch.int64, device=device)
    e = k % P
    off = (k // P) * pb + torch.from_numpy(poff).to(device)[e]
    ln = torch.from_numpy(pln.astype(np.int32)).to(device)[e]
    return arena, off, ln


class PeriodicSource:
    """One context whose borrowed arena is a periodic_source; use(m) attaches its first m payloads (the slots are back to back and the
    padding is clean, so the library takes the arena in place), release() gives the device memory back."""

    def __init__(self, patterns=(b"<K",)):
        self.m = GpuMatcher(0)
        self.m.set_patterns(list(patterns))
        self.keep = None

    def build(self, payloads, n):
        self.release()
        self.payloads, self.image, self.n = payloads, period_image(payloads), n
        self.keep = periodic_source(payloads, n)
        torch.cuda.synchronize()
        return self.use(n)

    def use(self, n):
        arena, off, ln = self.keep
        assert n <= self.n
        self.m.attach_arena(arena, off[:n], ln[:n], arena_bytes=periodic_end(self.image, n))
        return self.m

    def release(self):
        if self.keep is not None:
            self.m.load_arena(*EMPTY_ARENA)
            self.keep = None
            torch.cuda.empty_cache()

    def close(self):
        self.release()
        self.m.close()


def periodic_dst(image, index, n, period=PERIOD):
    """What a second arena has to hold that takes, of every period of a periodic source of n payloads, the entries `index` (ascending) as
    the packed image `image` = (bytes, off, len): `per` and `reps` -- the arena is `reps` times `per` --, `head`, the bytes of the last,
    incomplete period, `end`, and in full `off` uint64, `len` uint32 and `index` int64 (payload j of dst is payload index[j] of the
    source), all by index arithmetic."""
    img, poff, pln = image
    poff, pln, index = np.asarray(poff, dtype=np.int64), np.asarray(pln, dtype=np.int64), np.asarray(index, dtype=np.int64)
    assert len(poff) == len(pln) == len(index) and (np.diff(index) > 0).all() and (len(index) == 0 or index[-1] < period)
    reps, rest = divmod(n, period)
    pb = len(img)
    head = int((index < rest).sum())                                       # payloads of the incomplete period that dst holds
    hb = pb if head == len(pln) else int(poff[head])
    r = np.arange(reps, dtype=np.int64)[:, None]
    return {"per": img, "reps": reps, "head": img[:hb], "end": reps * pb + hb,
            "off": np.concatenate([(r * pb + poff[None, :]).ravel(), reps * pb + poff[:head]]).astype(np.uint64),
            "len": np.concatenate([np.tile(pln, reps), pln[:head]]).astype(np.uint32),
            "index": np.concatenate([(r * period + index[None, :]).ravel(), reps * period + index[:head]])}


def periodic_bytes(want):
    """the arena periodic_dst describes, in full (small inputs only)"""
    return np.concatenate([np.tile(want["per"], want["reps"]), want["head"]])


def check_periodic_bytes(a, want, rows=128):
    """A downloaded arena against periodic_dst's image, every byte: one reshape to [reps, period bytes] compared with the period's image
    `rows` rows at a time, the incomplete period's bytes, and the 64 bytes of 0x00 behind the end."""
    per, reps, end = want["per"], want["reps"], want["end"]
    pb = len(per)
    assert len(a) == end + 64, (len(a), end + 64)
    body = a[:reps * pb].reshape(reps, pb)
    for lo in range(0, reps, rows):
        blk = body[lo:lo + rows]
        if not (blk == per).all():
            r, c = (int(x) for x in np.argwhere(blk != per)[0])
            j = int(np.searchsorted(want["off"], (lo + r) * pb + c, side="right")) - 1
            raise AssertionError(f"{int((blk != per).sum())} bytes of periods {lo} .. {lo + len(blk) - 1} differ, the first at {(lo + r) * pb + c} = "
                                 f"period {lo + r} + {c}, payload {j} + {(lo + r) * pb + c - int(want['off'][j])}: {int(blk[r, c])}, not {int(per[c])}")
    bad = np.flatnonzero(a[reps * pb:end] != want["head"])
    assert bad.size == 0, (bad.size, reps * pb + int(bad[0]))
    assert not a[end:].any()


def tag_counts(payloads, times, n_tags=PERIOD):
    """counts[t] of prep_model.tag(t), t < n_tags, over an arena that holds payloads[j] times[j] times: a scan finds what stands in
    front of a payload's first 0x00"""
    want = np.zeros(n_tags, dtype=np.int64)
    for p, x in zip(payloads, times):
        if x:
            for m in PM._TAG.finditer(p.split(b"\0")[0]):
                if int(m.group(1)) < n_tags:
                    want[int(m.group(1))] += int(x)
    return want


# ------------------------------------------------------------------------------------------------
# frames: the library of tests/prep_model.py, and kmpgpu_load_frames over an index into it
# ------------------------------------------------------------------------------------------------
class FrameLib:
    """The frame library with the oracle's verdict on every frame under both rules."""

    def __init__(self, oracle):
        self.frames = PM.frame_library()
        self.blob, self.boff, self.cap = PM.library_blob(self.frames)
        self.K = len(self.frames)
        self.tags = [PM.tag(t) for t in range(self.K)]
        self.rule = {}
        for proto in ("udp", "tcp"):
            poff, plen = PM.library_rule(self.frames, proto, oracle.dump)
            self.rule[proto] = (poff, plen, PM.library_payloads(self.frames, poff, plen))


@pytest.fixture(scope="module")
def lib(oracle):
    return FrameLib(oracle)


def load_frames(gm, file_bytes, frame_off, caplen, proto, two_steps=False):
    G = _lib.gpu_lib()
    frame_off = np.ascontiguousarray(frame_off, dtype=np.uint64)
    caplen = np.ascontiguousarray(caplen, dtype=np.uint32)
    n = C.c_uint64(12345)
    args = (gm._ctx, file_bytes.ctypes.data_as(_lib.u8p), file_bytes.size, frame_off.ctypes.data_as(_lib.u64p), caplen.ctypes.data_as(_lib.u32p),
            len(frame_off), 1 if proto == "tcp" else 0)
    if two_steps:
        _lib.gpu_check(G.kmpgpu_load_frames_begin(*args), "kmpgpu_load_frames_begin")
        _lib.gpu_check(G.kmpgpu_load_frames_uploaded(gm._ctx), "kmpgpu_load_frames_uploaded")
        _lib.gpu_check(G.kmpgpu_load_frames_finish(gm._ctx, C.byref(n)), "kmpgpu_load_frames_finish")
    else:
        _lib.gpu_check(G.kmpgpu_load_frames(*args, C.byref(n)), "kmpgpu_load_frames")
    gm._keep = None
    return int(n.value)


# ------------------------------------------------------------------------------------------------
# flows
# ------------------------------------------------------------------------------------------------
FLOW_A, FLOW_B = 0x0A000001, 0xC0A80101
ONES = 0xFFFFFFFFFFFFFFFF


def meta_of_flows(flow, seed=1):
    """one record per payload for the flow numbers given: flow f talks from FLOW_A + f, port 1000 + f % 7, and every third payload of a
    flow is the answer (source and destination swapped)"""
    flow = np.asarray(flow, dtype=np.int64)
    rng = np.random.default_rng(seed)
    back = rng.integers(0, 3, len(flow)) == 0
    meta = np.zeros(len(flow), dtype=META_DTYPE)
    src, dst, sp, dp = FLOW_A + flow, np.full(len(flow), FLOW_B), 1000 + flow % 7, np.full(len(flow), 53)
    meta["src_ip"], meta["dst_ip"] = np.where(back, dst, src), np.where(back, src, dst)
    meta["src_port"], meta["dst_port"] = np.where(back, dp, sp), np.where(back, sp, dp)
    meta["proto"] = 17
    return meta


def check_fold(m, family, scope, want, counts=None):
    res = m.scan_flows(family, scope, hits=True)
    bad = np.argwhere(res["hits"] != want)
    assert bad.size == 0, [(int(r), int(f), bool(want[r, f])) for r, f in bad[:8]]
    assert res["flow_counts"].tolist() == want.sum(axis=1).tolist()
    assert res["any"].tolist() == want.any(axis=0).tolist()
    if counts is not None:
        assert res["counts"].tolist() == list(counts)
    # the raw words: the bits at n_flows and above are 0 in every word
    Wf = (want.shape[1] + 63) // 64
    hit_w, any_w = np.full((want.shape[0], Wf), ONES, dtype=np.uint64), np.full(Wf, ONES, dtype=np.uint64)
    fam = {"patterns": 0, "rules": 1, "relations": 2, "chains": 3}[family]
    _lib.gpu_check(m._g.kmpgpu_scan_flows(m._ctx, fam, 1 if scope == "flow" else 0, None, any_w.ctypes.data, hit_w.ctypes.data, None, None),
                   "kmpgpu_scan_flows")
    assert np.array_equal(hit_w, MM.words(want)) and np.array_equal(any_w, MM.words(want.any(axis=0)))
    return res


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
