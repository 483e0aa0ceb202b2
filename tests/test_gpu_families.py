"""The one row-family path of the C-ABI layer (csrc/kmpgpu.hip: scan_family, enqueue_family, family_rows) on the GPU: one context with
patterns, relations, chains, rules and windows set once goes through kmpgpu_scan_packets, _rules, _relations, _chains and the four
families of kmpgpu_scan_alerts, forwards and backwards, and every output equals the rows of tests/match_model.py / tests/chain_model.py.
The families share one marks buffer and one any[]: a call that read another family's rows, counts or any[], or what the call before
it left there, shows here.

Arenas of 64, 65 and 129 payloads: W = 1, 2, 3 words per row, on the device 2, 2, 4 -- the strided row download, the contiguous one, and
a padding word behind an odd row.

The same through the command lines (csrc/host/kmp_cli.c), whose output stage serves every file from one set of contexts: ONE run of
bin/serial and of bin/openmp_data with 3 shards with the offsets, packets, alerts and export files, rules that name a relation and a
chain, and windows all set at once.  udp_1000.pcap holds 1000 frames and 321 UDP payloads: the shards get 107 each, so the second one's
payload numbers start at an odd one.  The same run of bin/openmp_data once more with KMPGPU_DEVICE_EXTRACT=1, where the 1000 frames are
what is split -- 334 + 333 + 333, the remainder to shard 0 -- and the shards hold different numbers of payloads.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import DATA, GOLDEN  # noqa: E402

from gpu_support import gm, load, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import chain_model as CM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib, host  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    ALERT_CHAINS, ALERT_PATTERNS, ALERT_RELATIONS, ALERT_RULES, ALERTS_ALL, KERNEL_GENERAL, OPT_KERNEL, GpuMatcher)

EINVAL, ESTATE = -2, -3

PATS = [b"ab", b"cd", b"abc", b"Dab", b"b", b"cda"]
NOCASE = [False, True, False, True, False, False]
WINDOWS = [(0, 40), (2, None), (0, None), (0, 30), (1, 50), (0, None)]
RELATIONS = [(0, 1, 0, 6), (1, 0, None, 2), (4, 5, 1, None)]
CHAINS = [(0, (1, 0, 8), (4, 0, None)), (1, (0, None, 10))]
REL, CH = len(PATS), len(PATS) + len(RELATIONS)                # the first relation row, the first chain row
RULES = [([0], [1]), ([REL], []), ([CH], [REL + 1]), ([1, CH + 1], [2]), ([2, REL + 2], [5])]
SIZES = (64, 65, 129)

# (family of scan_alerts, its own call, the key of its per-row payload counts)
CALLS = (("patterns", "scan_packets", "pkt_counts"), ("rules", "scan_rules", "rule_pkt_counts"),
         ("relations", "scan_relations", "rel_pkt_counts"), ("chains", "scan_chains", "chain_pkt_counts"))


def payloads_of(n):
    rng = random.Random(f"families-{n}")
    return [bytes(rng.choice(b"abcdABCD") for _ in range(rng.randrange(0, 61))) for _ in range(n)]


@pytest.fixture(scope="module")
def models():
    """per arena size: the payloads, the model's rows per family and the totals; computed once"""
    out = {}
    for n in SIZES:
        payloads = payloads_of(n)
        st = MM.starts(payloads, PATS, windows=WINDOWS, nocase=NOCASE)
        hits = MM.hits(st)
        rel_rows = MM.relation_rows(st, PATS, RELATIONS)
        chain_rows = CM.chain_rows(st, PATS, CHAINS)
        rule_rows = MM.rule_rows(np.concatenate([hits, rel_rows, chain_rows]), RULES)
        rows = {"patterns": hits, "rules": rule_rows, "relations": rel_rows, "chains": chain_rows}
        for family, r in rows.items():                    # a bit to find and a bit to leave alone in every family
            assert r.any() and not r.all(), (n, family)
        out[n] = (payloads, rows, MM.counts(MM.starts(payloads, PATS, nocase=NOCASE)))        # every match, in window or not
    return out


def check_own_call(gm, call, key, rows, counts):
    res = getattr(gm, call)(hits=True)
    assert res["hits"].shape == rows.shape and np.array_equal(res["hits"], rows), call
    assert res[key].tolist() == rows.sum(axis=1).tolist(), call
    assert res["any"].tolist() == rows.any(axis=0).tolist(), call
    assert res["counts"].tolist() == counts, call


def check_alerts(gm, family, rows, counts):
    res = gm.scan_alerts(family)
    want = [(int(k), int(i)) for k, i in np.argwhere(rows.T)]
    assert list(zip(res["alerts"]["packet"].tolist(), res["alerts"]["index"].tolist())) == want, family
    assert res["n_found"] == len(want) and res["n_packets"] == int(rows.any(axis=0).sum()), family
    assert res["pkt_counts"].tolist() == rows.sum(axis=1).tolist(), family
    assert res["counts"].tolist() == counts, family


def test_one_context_through_all_five_calls(gm, models):
    try:
        reset(gm)
        gm.set_patterns(PATS, nocase=NOCASE)
        gm.set_relations(RELATIONS)
        gm.set_chains(CHAINS)
        gm.set_rules(RULES)
        gm.set_windows(WINDOWS)
        for n in SIZES:
            payloads, rows, counts = models[n]
            load(gm, payloads)
            steps = [("own", c) for c in CALLS] + [("alerts", c) for c in CALLS]
            for kind, (family, call, key) in steps + steps[::-1]:
                if kind == "own":
                    check_own_call(gm, call, key, rows[family], counts)
                else:
                    check_alerts(gm, family, rows[family], counts)
    finally:
        reset(gm)


def test_precondition_order():
    """which precondition speaks where two fail at once, through the raw C calls: the return code, and kmpgpu_last_error names the call"""
    g = _lib.gpu_lib()
    scans = {name: getattr(g, "kmpgpu_scan_" + name) for name in ("packets", "rules", "relations", "chains")}

    def own(m, name):
        rc = scans[name](m._ctx, None, None, None, None, None)
        return rc, g.kmpgpu_last_error().decode().startswith(f"kmpgpu_scan_{name}")

    def alerts(m, family):
        found = C.c_uint64()
        rc = g.kmpgpu_scan_alerts(m._ctx, family, ALERTS_ALL, C.byref(found), None, None, None, None)
        return rc, g.kmpgpu_last_error().decode().startswith("kmpgpu_scan_alerts")

    with GpuMatcher(0) as m:
        m.set_option(OPT_KERNEL, KERNEL_GENERAL)
        # the general kernel and no patterns: the marking pass checks the kernel first
        assert own(m, "packets") == (EINVAL, True)
        assert alerts(m, ALERT_PATTERNS) == (EINVAL, True)
        # the general kernel, patterns, nothing of the family: the family's own check comes before the marking pass
        m.set_patterns(PATS, nocase=NOCASE)
        for name, family in (("rules", ALERT_RULES), ("relations", ALERT_RELATIONS), ("chains", ALERT_CHAINS)):
            assert own(m, name) == (ESTATE, True), name
            assert alerts(m, family) == (ESTATE, True), name
        # everything set: the kernel is what is left to refuse
        m.set_relations(RELATIONS)
        m.set_chains(CHAINS)
        m.set_rules(RULES)
        m.set_windows(WINDOWS)
        load(m, payloads_of(SIZES[0]))
        for name, family in (("packets", ALERT_PATTERNS), ("rules", ALERT_RULES), ("relations", ALERT_RELATIONS), ("chains", ALERT_CHAINS)):
            assert own(m, name) == (EINVAL, True), name
            assert alerts(m, family) == (EINVAL, True), name


# ------------------------------------------------------------------------------------------------
# the command lines: every output file from one run
# ------------------------------------------------------------------------------------------------
CLI_SHARDS = 3


@pytest.fixture(scope="module")
def cli_case(tokens, tmp_path_factory):
    """the windows, relations, chains and rules files, and what tests/match_model.py says each output file holds; computed once"""
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(arena.payload(k)) for k in range(arena.n_pkts)]
    N, H, I, X, L, U = (tokens.index(t) for t in (b"NOTIFY", b"http", b"id", b"xml", b"LOCATION", b"Linux"))
    n = len(tokens)
    windows = [(0, None)] * n
    for i, w in ((N, (0, 0)), (H, (0, 100)), (I, (60, None)), (U, (0, 199))):
        windows[i] = w
    relations = [(L, H, 2, 2), (H, X, None, 34)]
    chains = [(N, (H, 70, 100), (X, None, 34)), (X, (U, 48, 80))]
    rel, ch = n, n + len(relations)                                       # the first relation row, the first chain row
    rules = [([N], [U, L]), ([rel], [rel + 1]), ([ch, I], [L]), ([ch + 1, rel + 1], [])]

    def star(x):
        return "*" if x is None else str(x)

    def term(i):
        return str(i) if i < rel else f"r{i - rel}" if i < ch else f"c{i - ch}"

    d = tmp_path_factory.mktemp("cli_all")
    (d / "windows.txt").write_text("# pattern first last\n" + "".join(f"{i} {a} {star(b)}\n" for i, (a, b) in enumerate(windows) if (a, b) != (0, None)))
    (d / "relations.txt").write_text("".join(f"{a} {b} {star(lo)} {star(hi)}\n" for a, b, lo, hi in relations))
    (d / "chains.txt").write_text("".join(str(c[0]) + "".join(f" {star(lo)} {star(hi)} {p}" for p, lo, hi in c[1:]) + "\n" for c in chains))
    (d / "rules.txt").write_text("\n".join(" ".join([term(i) for i in pos] + ["!" + term(i) for i in neg]) for pos, neg in rules) + "\n")

    free = MM.starts(payloads, tokens)
    st = MM.starts(payloads, tokens, windows)
    hits = MM.hits(st)
    rows = MM.rule_rows(np.concatenate([hits, MM.relation_rows(st, tokens, relations), CM.chain_rows(st, tokens, chains)]), rules)
    want = {"offsets": sorted(MM.records(st)),
            "packets": sorted((int(k), int(i)) for i, k in np.argwhere(hits)),
            "alerts": sorted((int(k), int(r)) for r, k in np.argwhere(rows)),
            "export": [payloads[int(k)] for k in np.flatnonzero(rows.any(axis=0))]}
    # by the model: every file has something from each of the three shards, the windows take matches away, the rules -- each of which
    # matches somewhere -- select some of the payloads that hold a pattern, not all
    assert len(payloads) % CLI_SHARDS == 0
    per = len(payloads) // CLI_SHARDS
    assert per % 2 == 1
    for name in ("offsets", "packets", "alerts"):
        assert {rec[0] // per for rec in want[name]} == set(range(CLI_SHARDS)), name
    assert {int(k) // per for k in np.flatnonzero(rows.any(axis=0))} == set(range(CLI_SHARDS))
    assert len(want["offsets"]) < len(MM.records(free)) and rows.any(axis=1).all()
    assert 0 < len(want["export"]) < int(MM.hits(free).any(axis=0).sum())
    # with the extraction on the device the FRAMES are split, N / P each and the remainder to shard 0: the shards' payload counts differ,
    # and again every file has something from each shard
    is_payload = [host.extract(frame, caplen, "udp") is not None for caplen, _, frame in host.read_pcap(os.path.join(DATA, "udp_1000.pcap"))]
    n_frames = len(is_payload)
    assert n_frames % CLI_SHARDS != 0 and sum(is_payload) == len(payloads)
    cuts = [0, n_frames // CLI_SHARDS + n_frames % CLI_SHARDS, 2 * (n_frames // CLI_SHARDS) + n_frames % CLI_SHARDS, n_frames]
    lo = [sum(is_payload[:c]) for c in cuts]                              # the first payload of every frame shard
    assert len({b - a for a, b in zip(lo, lo[1:])}) == CLI_SHARDS

    def frame_shard(k):
        return sum(k >= x for x in lo[1:-1])

    for name in ("offsets", "packets", "alerts"):
        assert {frame_shard(rec[0]) for rec in want[name]} == set(range(CLI_SHARDS)), name
    assert {frame_shard(int(k)) for k in np.flatnonzero(rows.any(axis=0))} == set(range(CLI_SHARDS))
    return d, want


@pytest.fixture(scope="module")
def cli_all(cli_case):
    """(prog, extract) -> the bytes of the four files of its one run; it runs once, whichever test asks first"""
    d, _ = cli_case
    done = {}

    def files_of(prog, extra, extract=False):
        if (prog, extract) not in done:
            out = {name: d / f"{prog}_{int(extract)}_{name}" for name in ("offsets", "packets", "alerts", "export")}
            r = run_cli(prog, extra=extra, env_extra={"KMPGPU_DEVICE_EXTRACT": "1" if extract else "0",
                                                      "KMPGPU_WINDOWS_FILE": str(d / "windows.txt"), "KMPGPU_RELATIONS_FILE": str(d / "relations.txt"),
                                                      "KMPGPU_CHAINS_FILE": str(d / "chains.txt"), "KMPGPU_RULES_FILE": str(d / "rules.txt"),
                                                      "KMPGPU_OFFSETS_FILE": str(out["offsets"]), "KMPGPU_PACKETS_FILE": str(out["packets"]),
                                                      "KMPGPU_ALERTS_FILE": str(out["alerts"]), "KMPGPU_EXPORT_FILE": str(out["export"])})
            assert r.returncode == 0, r.stderr
            with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
                assert strip_elapsed(r.stdout) == f.read()                    # the counts follow none of the variables
            done[prog, extract] = {name: path.read_bytes() for name, path in out.items()}
        return done[prog, extract]

    return files_of


@pytest.mark.parametrize("prog,extra,extract,other", [("serial", [], False, ("openmp_data", [str(CLI_SHARDS)])), ("openmp_data", [str(CLI_SHARDS)], False, ("serial", [])),
                                                      ("openmp_data", [str(CLI_SHARDS)], True, ("serial", []))],
                         ids=["serial", "openmp_data-3", "openmp_data-3-device_extract"])
def test_cli_every_output_file_from_one_run(cli_case, cli_all, tmp_path, prog, extra, extract, other):
    d, want = cli_case
    got = cli_all(prog, extra, extract)

    def records(name):
        return [tuple(int(x) for x in line.split(",")) for line in got[name].decode().splitlines()]

    assert sorted(records("offsets")) == want["offsets"]                          # (the order of the matches is unspecified: kmpgpu_scan_offsets)
    assert records("packets") == want["packets"]
    assert records("alerts") == want["alerts"]
    back_path = tmp_path / "export.pcap"
    back_path.write_bytes(got["export"])
    back = K.HostArena.from_pcap(str(back_path), "udp")
    assert [bytes(back.payload(k)) for k in range(back.n_pkts)] == want["export"]   # exactly the payloads of the rules' any
    # the same bytes from the other program; the offsets file as a set of lines, its order being what it is
    theirs = cli_all(*other)
    for name in ("packets", "alerts", "export"):
        assert got[name] == theirs[name], name
    assert sorted(got["offsets"].splitlines()) == sorted(theirs["offsets"].splitlines())
