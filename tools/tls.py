"""What the TLS ClientHello buffers cost: kmpgpu_tls_locate against kmpgpu_dns_locate and kmpgpu_http_locate on the same arena,
kmpgpu_load_tls for both fields against kmpgpu_load_dns and kmpgpu_load_selected, and the unchanged calls against the parent commit's
library (profiles/tls.txt).

    python3 tools/tls.py [--parent-lib <libkmpgpu.so of the parent commit>] [--reps 20] [--out profiles/tls.txt]

kernel_ms of kmpgpu_last_timing, medians of --reps repeats after a warm-up, the calls of a section taking turns inside each round so
that drift hits them alike.
  (1) no TLS           1 M payloads of 1 500 bytes of lower-case letters: the first unit rules every payload out.  The arena is attached
                       anew before every call, which drops all spans.  In the same rounds: kmpgpu_dns_locate and kmpgpu_http_locate.
  (2) hellos           1 M ClientHellos of about 200 bytes (8 extensions) and of 517 bytes (12 extensions, the last one padding), a pool
                       of 4 096 repeated, every one with a server name and an ALPN list.
  (3) the load         kmpgpu_load_tls for sni and alpn over the 517-byte hellos with valid spans, against kmpgpu_load_selected of the
                       same payloads, and against kmpgpu_load_dns over 1 M DNS messages of 40 to 120 bytes (tools/dns.py's arena), in
                       the same rounds.
  (4) unchanged calls  kmpgpu_scan_rules (strings.txt's tokens, 100 generated rules, 1 M x 1 500 B) and kmpgpu_load_dns over the DNS
                       messages: (a) the parent's library, (b) this tree's; unchanged: (b)'s median inside (a)'s own range of the run.
                       Left out without --parent-lib."""
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
from multithreading_string_matching_amd.matcher import DNS_QNAME, TLS_ALPN, TLS_SNI, GpuMatcher  # noqa: E402

from dns import pooled_arena as dns_arena  # noqa: E402  (tools/dns.py: the arena of DNS messages)
from fields import L, make_arena  # noqa: E402  (tools/fields.py: the arenas of 1 500-byte payloads)
from headers import gen_rules, matcher_on, spread  # noqa: E402  (tools/headers.py: the same instrument)

POOL = 4096
HOST = b"abcdefghijklmnopqrstuvwxyz0123456789-"


def ext(ty, body):
    return struct.pack(">HH", ty, len(body)) + body


def hello(rng, size):
    """a ClientHello as a TLS 1.3 client writes it: 32-byte session id, 15 suites, server name, ALPN h2 / http/1.1 and other extensions
    as opaque bytes; size: None, or the record's size, reached with a padding extension (type 21) as OpenSSL does"""
    host = b".".join(bytes(rng.choice(HOST) for _ in range(rng.randrange(3, 12))) for _ in range(rng.randrange(2, 4)))
    sni = struct.pack(">HBH", len(host) + 3, 0, len(host)) + host
    alpn = b"\x02h2\x08http/1.1"
    exts = [ext(0, sni), ext(11, b"\x03\x00\x01\x02"), ext(10, bytes(rng.randrange(256) for _ in range(14))), ext(35, b""),
            ext(16, struct.pack(">H", len(alpn)) + alpn), ext(22, b""), ext(23, b""), ext(13, bytes(rng.randrange(256) for _ in range(rng.randrange(20, 34))))]
    if size is not None:
        exts += [ext(43, b"\x04\x03\x04\x03\x03"), ext(45, b"\x01\x01"), ext(51, bytes(rng.randrange(256) for _ in range(38)))]
    fixed = b"\x03\x03" + bytes(rng.randrange(256) for _ in range(32)) + b"\x20" + bytes(rng.randrange(256) for _ in range(32)) + \
        struct.pack(">H", 30) + bytes(rng.randrange(256) for _ in range(30)) + b"\x01\x00"
    xs = b"".join(exts)
    if size is not None:
        xs += ext(21, bytes(size - 9 - len(fixed) - 2 - len(xs) - 4))
    body = fixed + struct.pack(">H", len(xs)) + xs
    msg = b"\x01" + struct.pack(">I", len(body))[1:] + body
    return b"\x16\x03\x01" + struct.pack(">H", len(msg)) + msg


def pooled(n, pool):
    """n payloads, payload k = pool entry k % POOL, packed with clean padding, on the device: (arena, off int64, len int32, payload bytes)"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tls.txt"))
    args = ap.parse_args()
    n = args.payloads
    lines = [f"TLS ClientHello buffers (kmpgpu_tls_locate, kmpgpu_load_tls), {n} payloads, kernel_ms, medians of {args.reps} alternating repeats with "
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

    src, dst, sel, names, qn = (GpuMatcher(0) for _ in range(5))
    parent = matcher_on(args.parent_lib) if args.parent_lib else None
    g = dst._g
    try:
        off15, ln15, _ = K.arena_layout(None, L, n)
        letters = (make_arena(n, "no HTTP"), torch.from_numpy(off15.astype(np.int64)).cuda(), torch.from_numpy(ln15.astype(np.int32)).cuda(), n * L)
        rng = random.Random(11)
        short = pooled(n, [hello(rng, None) for _ in range(POOL)])
        full = pooled(n, [hello(rng, 517) for _ in range(POOL)])
        torch.cuda.synchronize()

        def locate(arena, which):
            src.attach_arena(*arena[:3])                             # drops the spans
            st = {"tls": src.tls_locate, "dns": src.dns_locate, "http": src.http_locate}[which]()
            t = src.last_timing()
            assert t.launches == 1
            return t.kernel_ms, st

        _, st = locate(letters, "tls")
        assert st["n_hellos"] == 0
        t = by_turns({key: (lambda key=key: locate(letters, key)[0]) for key in ("tls", "dns", "http")})
        mt, md, mh = (statistics.median(t[key]) for key in ("tls", "dns", "http"))
        say(f"(1) {L} bytes of letters, no TLS: kmp_tls_locate_kernel {spread(t['tls'])} ({n / mt / 1e6:.2f} G payloads/s); kmp_dns_locate_kernel "
            f"{spread(t['dns'])}; kmp_http_locate_kernel {spread(t['http'])}; tls / dns {mt / md:.3f}; tls / http {mt / mh:.3f}")
        for kind, arena in (("about 200 bytes", short), ("517 bytes", full)):
            _, st = locate(arena, "tls")
            assert st["n_hellos"] == st["n_sni"] == st["n_alpn"] == n and st["n_truncated"] == 0
            t = by_turns({"tls": lambda: locate(arena, "tls")[0]})
            mt = statistics.median(t["tls"])
            say(f"(2) ClientHellos of {kind} ({arena[3] / n:.0f} on average): kmp_tls_locate_kernel {spread(t['tls'])} ({n / mt / 1e6:.2f} G payloads/s)")

        src.attach_arena(*full[:3])
        src.tls_locate()
        d_a, d_o, d_l, nb = dns_arena(n, False)
        names.attach_arena(d_a, d_o, d_l)
        names.dns_locate()
        ones = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
        n_out = C.c_uint64()
        fst = _lib.FieldsStats()

        def load_tls(field):
            assert g.kmpgpu_load_tls(dst._ctx, src._ctx, field, 0, None, None, C.byref(fst)) == 0 and fst.n_present == n
            t = dst.last_timing()
            assert t.launches == 5
            return t.kernel_ms

        def load_dns(lib=g, d=qn, s=names):
            assert lib.kmpgpu_load_dns(d._ctx, s._ctx, DNS_QNAME, 0, None, None, C.byref(fst)) == 0 and fst.n_present == n
            t = d.last_timing()
            assert t.launches == 5
            return t.kernel_ms

        def selected():
            assert g.kmpgpu_load_selected(sel._ctx, src._ctx, ones.data_ptr(), 1, C.byref(n_out)) == 0 and n_out.value == n
            return sel.last_timing().kernel_ms

        t = by_turns({"sni": lambda: load_tls(TLS_SNI), "alpn": lambda: load_tls(TLS_ALPN), "load_dns": load_dns, "load_selected": selected})
        ms, md = statistics.median(t["load_selected"]), statistics.median(t["load_dns"])
        for key, field in (("sni", TLS_SNI), ("alpn", TLS_ALPN)):
            load_tls(field)
            mf = statistics.median(t[key])
            say(f"(3) kmpgpu_load_tls {key}: {int(fst.bytes_out)} field bytes of {int(fst.bytes_in)}; kernel_ms {spread(t[key])}; / load_selected "
                f"{mf / ms:.3f}; / load_dns {mf / md:.3f}")
        load_dns()
        say(f"(3) kmpgpu_load_dns, {n} DNS messages: {int(fst.bytes_out)} name bytes of {int(fst.bytes_in)}; kernel_ms {spread(t['load_dns'])}")
        say(f"(3) kmpgpu_load_selected, all {n} hellos: kernel_ms {spread(t['load_selected'])} ({2 * full[3] / ms / 1e6:.0f} GB/s over one read and one write)")

        if parent is not None:
            tokens = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
            rules = gen_rules(random.Random(100), 100, len(tokens))
            d_w = make_arena(n, "blank line in the first 256 bytes")
            ms = {"a": parent, "b": sel}
            for m in ms.values():
                m.set_patterns(tokens)
                m.attach_arena(d_w, letters[1], letters[2])
                m.set_rules(rules)
            res = {key: m.scan_rules(hits=True) for key, m in ms.items()}
            assert all(np.array_equal(res["a"][k], res["b"][k]) for k in ("hits", "any", "counts", "rule_pkt_counts"))

            def compare(label, calls):
                t = by_turns(calls)
                ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
                say(f"(4) {label}: (a) parent {spread(t['a'])}; (b) this tree {spread(t['b'])}; (b) / (a) {mb / ma:.4f}; the parent's range "
                    f"{min(t['a']):.3f} .. {max(t['a']):.3f}, (b)'s median inside it: {'yes' if min(t['a']) <= mb <= max(t['a']) else 'NO'}")

            compare(f"kmpgpu_scan_rules, {len(tokens)} tokens, {len(rules)} rules", {key: (lambda m=m: m.scan_rules()["timing"].kernel_ms) for key, m in ms.items()})
            srcs = {"a": matcher_on(args.parent_lib), "b": names}
            dsts = {"a": matcher_on(args.parent_lib), "b": qn}
            srcs["a"].attach_arena(d_a, d_o, d_l)
            srcs["a"].dns_locate()
            compare("kmpgpu_load_dns", {key: (lambda key=key: load_dns(srcs[key]._g, dsts[key], srcs[key])) for key in srcs})
            assert all(np.array_equal(x, y) for x, y in zip(dsts["a"].arena_download(), dsts["b"].arena_download()))
            assert srcs["a"].dns_spans().tobytes() == srcs["b"].dns_spans().tobytes()
            dsts["a"].close()
            srcs["a"].close()
    finally:
        for m in (src, dst, sel, names, qn, parent):
            if m is not None:
                m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
