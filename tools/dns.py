"""What the DNS query-name buffers cost: kmpgpu_dns_locate against kmpgpu_http_locate on the same arenas, kmpgpu_load_dns against
kmpgpu_load_fields(raw_uri) and kmpgpu_load_selected with all bits set, and the unchanged calls against the parent commit's library
(profiles/dns.txt).

    python3 tools/dns.py [--parent-lib <libkmpgpu.so of the parent commit>] [--reps 20] [--out profiles/dns.txt]

kernel_ms of kmpgpu_last_timing, medians of --reps repeats after a warm-up, the calls of a section taking turns inside each round so
that drift hits them alike.
  (1) the locate       three arenas of 1 M payloads: (a) DNS messages of 40 to 120 bytes with names of 1 to 6 labels, a pool of 4 096
                       repeated; (b) 1 500 bytes of lower-case letters each, no DNS: the first unit rules every payload out; (c) root
                       questions of 17 bytes.  The arena is attached anew before every call, which drops both kinds of spans.  In the
                       same rounds: kmpgpu_http_locate, which finds next to no message in any of the three, so it reads one unit per payload.
  (2) the load         kmpgpu_load_dns over arena (a) with valid spans, against kmpgpu_load_selected of all payloads of (a) and against
                       kmpgpu_load_fields(raw_uri) over 1 M requests of 1 500 bytes (tools/fields.py's arena), in the same rounds.
  (3) unchanged calls  kmpgpu_scan_rules (strings.txt's tokens, 100 generated rules) and kmpgpu_load_fields(raw_uri) over the requests:
                       (a) the parent's library, (b) this tree's; unchanged: (b)'s median inside (a)'s own range of the run.  Left out
                       without --parent-lib."""
import argparse
import ctypes as C
import os
import random
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: see tests/test_gpu_parity.py)

import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import DNS_QNAME, FIELD_RAW_URI, GpuMatcher  # noqa: E402

from fields import L, make_arena  # noqa: E402  (tools/fields.py: the arenas of 1 500-byte payloads)
from headers import gen_rules, matcher_on, spread  # noqa: E402  (tools/headers.py: the same instrument)

POOL = 4096


def message(rng, root):
    labels = [] if root else [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789-") for _ in range(rng.randrange(2, 13))) for _ in range(rng.randrange(1, 7))]
    wire = b"".join(bytes([len(x)]) + x for x in labels) + b"\x00"
    msg = struct.pack(">6H", rng.randrange(65536), rng.choice((0x0100, 0x8180)), 1, 0, 0, 0) + wire + b"\x00\x01\x00\x01"
    if not root:
        msg += bytes(rng.randrange(256) for _ in range(max(0, rng.randrange(40, 121) - len(msg))))
    return msg


def pooled_arena(n, root):
    """n payloads, payload k = pool entry k % POOL, packed with clean padding, on the device: (arena, off int64, len int32, name bytes)"""
    rng = random.Random(7 if root else 8)
    pool = [message(rng, root) for _ in range(POOL)]
    ln = np.array([len(t) for t in pool], dtype=np.int64)
    slot = np.maximum(16, (ln + 15) & ~15)
    poff = np.cumsum(slot) - slot
    img = np.zeros(int(slot.sum()), dtype=np.uint8)
    for o, t in zip(poff.tolist(), pool):
        img[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    assert n % POOL == 0
    reps = n // POOL
    arena = torch.cat([torch.from_numpy(img).cuda().repeat(reps), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    k = torch.arange(n, dtype=torch.int64, device="cuda")
    off = (k // POOL) * len(img) + torch.from_numpy(poff).cuda()[k % POOL]
    d_len = torch.from_numpy(ln.astype(np.int32)).cuda()[k % POOL]
    return arena, off, d_len, int(ln.sum()) * reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--payloads", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dns.txt"))
    args = ap.parse_args()
    n = args.payloads
    lines = [f"DNS query-name buffers (kmpgpu_dns_locate, kmpgpu_load_dns), {n} payloads, kernel_ms, medians of {args.reps} alternating repeats with "
             f"min / quartiles / max, ms (GPU: {torch.cuda.get_device_name(0)}); parent library: {'yes' if args.parent_lib else 'none given'}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def by_turns(calls, reps=args.reps):
        t = {key: [] for key in calls}
        for rnd in range(3 + reps):
            for key, fn in calls.items():
                x = fn()
                if rnd >= 3:
                    t[key].append(x)
        return t

    src, dst, sel, web, uri = (GpuMatcher(0) for _ in range(5))
    parent = matcher_on(args.parent_lib) if args.parent_lib else None
    g = dst._g
    try:
        off15, ln15, _ = K.arena_layout(None, L, n)
        letters = (make_arena(n, "no HTTP"), torch.from_numpy(off15.astype(np.int64)).cuda(), torch.from_numpy(ln15.astype(np.int32)).cuda(), n * L)
        arenas = {"DNS messages of 40 to 120 bytes": pooled_arena(n, False), f"{L} bytes of letters, no DNS": letters,
                  "root questions of 17 bytes": pooled_arena(n, True)}
        torch.cuda.synchronize()
        for kind, (d_a, d_o, d_l, nb) in arenas.items():
            def locate(http):
                src.attach_arena(d_a, d_o, d_l)                      # drops the spans
                st = src.http_locate() if http else src.dns_locate()
                t = src.last_timing()
                assert t.launches == 1
                return t.kernel_ms, st

            _, st = locate(False)
            _, hst = locate(True)
            t = by_turns({"dns": lambda: locate(False)[0], "http": lambda: locate(True)[0]})
            md, mh = statistics.median(t["dns"]), statistics.median(t["http"])
            say(f"(1) {kind}: {st['n_queries']} queries, {st['n_responses']} responses, {st['n_root']} root names, {st['name_bytes']} name bytes of {nb} "
                f"payload bytes; kmp_dns_locate_kernel {spread(t['dns'])} ({n / md / 1e6:.2f} G payloads/s); kmp_http_locate_kernel ({hst['bytes_scanned']} bytes "
                f"scanned) {spread(t['http'])}; dns / http {md / mh:.3f}")

        d_a, d_o, d_l, nb = arenas["DNS messages of 40 to 120 bytes"]
        src.attach_arena(d_a, d_o, d_l)
        src.dns_locate()
        d_w = make_arena(n, "blank line in the first 256 bytes")
        web.attach_arena(d_w, letters[1], letters[2])
        web.http_locate()
        ones = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
        n_out = C.c_uint64()
        fst = _lib.FieldsStats()

        def names():
            assert g.kmpgpu_load_dns(dst._ctx, src._ctx, DNS_QNAME, 0, None, None, C.byref(fst)) == 0 and fst.n_present == n
            t = dst.last_timing()
            assert t.launches == 5
            return t.kernel_ms

        def raw_uri(lib=g, d=uri, s=web):
            assert lib.kmpgpu_load_fields(d._ctx, s._ctx, FIELD_RAW_URI, 0, None, None, C.byref(fst)) == 0 and fst.n_present == n
            t = d.last_timing()
            assert t.launches == 5
            return t.kernel_ms

        def selected():
            assert g.kmpgpu_load_selected(sel._ctx, src._ctx, ones.data_ptr(), 1, C.byref(n_out)) == 0 and n_out.value == n
            return sel.last_timing().kernel_ms

        t = by_turns({"load_dns": names, "raw_uri": raw_uri, "load_selected": selected})
        names()
        say(f"(2) kmpgpu_load_dns: {int(fst.bytes_out)} name bytes of {int(fst.bytes_in)}; kernel_ms {spread(t['load_dns'])}; / load_selected "
            f"{statistics.median(t['load_dns']) / statistics.median(t['load_selected']):.3f}; / load_fields(raw_uri) "
            f"{statistics.median(t['load_dns']) / statistics.median(t['raw_uri']):.3f}")
        raw_uri()
        say(f"(2) kmpgpu_load_fields raw_uri, {n} x {L} B: {int(fst.bytes_out)} field bytes of {int(fst.bytes_in)}; kernel_ms {spread(t['raw_uri'])}")
        say(f"(2) kmpgpu_load_selected, all {n} DNS messages: kernel_ms {spread(t['load_selected'])} "
            f"({2 * nb / statistics.median(t['load_selected']) / 1e6:.0f} GB/s over one read and one write)")

        if parent is not None:
            tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
            rules = gen_rules(random.Random(100), 100, len(tokens))
            ms = {"a": parent, "b": web}
            for m in ms.values():
                m.set_patterns(tokens)
                m.attach_arena(d_w, letters[1], letters[2])
                m.set_rules(rules)
            res = {key: m.scan_rules(hits=True) for key, m in ms.items()}
            assert all(np.array_equal(res["a"][k], res["b"][k]) for k in ("hits", "any", "counts", "rule_pkt_counts"))

            def compare(label, calls):
                t = by_turns(calls)
                ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
                say(f"(3) {label}: (a) parent {spread(t['a'])}; (b) this tree {spread(t['b'])}; (b) / (a) {mb / ma:.4f}; the parent's range "
                    f"{min(t['a']):.3f} .. {max(t['a']):.3f}, (b)'s median inside it: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}")

            compare(f"kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules", {key: (lambda m=m: m.scan_rules()["timing"].kernel_ms) for key, m in ms.items()})
            dsts = {"a": matcher_on(args.parent_lib), "b": uri}
            for m in ms.values():
                m.http_locate()
            compare("kmpgpu_load_fields raw_uri", {key: (lambda key=key: raw_uri(ms[key]._g, dsts[key], ms[key])) for key in ms})
            assert all(np.array_equal(x, y) for x, y in zip(dsts["a"].arena_download(), dsts["b"].arena_download()))
            dsts["a"].close()
    finally:
        for m in (src, dst, sel, web, uri, parent):
            if m is not None:
                m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
