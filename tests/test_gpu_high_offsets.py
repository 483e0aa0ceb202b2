"""Everything behind the marking pass, and the loaders, on payloads in front of, across and behind arena offset 2^32, on a real MI355X.

The shape the project is built for -- 8 M payloads of 1500 bytes, a 12 GB arena -- has almost every payload above 2^32, and the suite
reached such offsets with the counting flat and packed kernels, the extraction and the select copy only.  Here one world of 600 payloads
is attached inside ONE borrowed buffer that starts at offset 0 and is a little over 4 GiB long (gpu_support.big_buffer, attach_placed),
at four places (gpu_support.placed_base):
    low     base 0: the control, which tells "the world is wrong" from "the placement is wrong"
    split   2^32 lies inside payload SPLIT_K, 48 bytes of it in front; SPLIT_K % 64 = 37 and 306 payloads follow: the wavefront of a
            per-payload kernel that holds it has lanes on both sides
    edge    a slot ends at 2^32 and payload EDGE_K starts there
    behind  base 2^32 + 4096 + 48: every offset above 2^32, the first payload on no 128-byte line (the streaming kernels' head lanes)
Every expectation comes from the host models (match_model, chain_model, bytetest_model, regex_model, header_model, flow_model, seam_model,
prep_model) and the CPU oracle, none depends on the placement, and every comparison is exact.  tests/test_gpu_scan_matrix.py runs every
scan-kernel instantiation at the same placements (test_row_placed).

What is planted (World, asserted on the CPU before anything runs): in SPLIT_K and in every fifth longer payload, from byte 40 on,
"GET", three bytes, "HoSt", "key=" -- so that under `split` a nocase match ("host", bytes 46..49) holds byte 2^32, a relation's and a
chain link's first content ends in front of it and the next one starts behind it, the 4-byte field of an absolute byte test is bytes
2^32 - 2 .. 2^32 + 1 (read in both byte orders), a relative byte test has its anchor in front and its field behind, and a $-anchored
expression and one of 49 positions from ^ on have matches that hold it.  (`^.{46}..` alone ends at byte 47, the last one in front; the
expression here asks for one byte more.)  A pattern of reach + 1 = 99 bytes is cut in two by the end of SPLIT_K and goes on in the next
payload of its flow direction: the flow holds it across that seam only.  Every row of every family has a set and an unset bit among the
payloads in front of SPLIT_K and behind it, and in front of EDGE_K and from it on: a kernel that read zeros for every high payload
could not pass on empty rows.

Address arithmetic read before the first run, for offsets of 2^32 and more (csrc/):
    kmp_scan_stream_kernels.inc  flat: base = arena + k0 * (uint64_t)stride, arena moved by uni_off0 on the host; range 32-bit by
                                 grid_blocks' bound.  packed: off0 = plan[gw].off - pre in 64 bits, make_rsrc(arena + off0, range) takes the
                                 low word and 16 bits of the high one, range = plan[gw + 1].off - off0 < 2^31 by the planner; the bitmap
                                 index (off0 >> 4) >> 6 and p0 = (uint32_t)(off0 + cb + vo0 - po) are 64-bit differences.  Clean.
    kmp_scan_stream.hip          kmp_build_bitmap_kernel: slot = pkt_off[k] >> 4 as uint64 (slot numbers from 2^28 on), word slot >> 6;
                                 kmp_plan_kernel: 64-bit targets and binary search.  Clean.
    kmp_scan_multi.hip           blk_off0 rebuilt from two 32-bit halves, to_end = span_end - blk_off0 clamped to 0x7FFF0000 for the
                                 resource, bitmap + (blk_off0 >> 10), unit entries as 32-bit differences to blk_off0.  Clean.
    kmp_scan_general.hip         it.off / it.off_n uint64, base = arena + it.off as a scalar pair, 32-bit offsets inside the payload.  Clean.
    kmp_sweep_dev.h, kmp_relations.hip, kmp_chains.hip, kmp_bytetests.hip
                                 off = pkt_off[k] uint64 per wavefront, text_end / match_at / bytetest_holds take arena + off (and
                                 fold + off); the absolute byte-test kernel text = arena + pkt_off[k] per lane.  Clean.
    kmp_regex.hip                text = arena + pkt_off[k] per lane, p a 32-bit position inside the payload.  Clean.
    kmp_seams.hip                index kernel: ts = src_off[p] + Lp - tail and hs in 64 bits, stored as two 32-bit halves of the 32-byte
                                 record and put together again by the gather; fetch_piece adds a small signed start to a 64-bit base.  Clean.
    kmp_select.hip               src + s_src[wid][p] + rel with s_src uint64 (tests/test_gpu_select.py has its own high source).  Clean.
    kmp_fold.hip                 vector index uint64 from blockIdx.x * 1024, 2^18 blocks for 4 GiB; kmp_slot_end_kernel 64-bit sums.  Clean.
    kmp_prep.hip                 repack / gather, check_padding (arena + pkt_off[k] + (L - r)), effective_bytes (arena + pkt_off[k]),
                                 validate (o > arena_bytes || slot > arena_bytes - o in 64 bits).  Clean.
Nothing was found by reading, so nothing was changed in csrc/.

Not reached: the flat -> packed -> general fallbacks at ppw * stride >= 2^31 and bpw >= 2^30 need arenas of a TiB under the grids of the
tests.

Memory: the module's buffer is 4 GiB + 8 MiB, made once; the patterns hold nocase ones, so the library's fold buffer of the first
context adds up to 4 GiB (arena_bytes is base + the end of the last slot): a peak of a little over 8 GiB, plus 32 MiB of start bitmap.

Run on a real MI355X:  python -m pytest tests/test_gpu_high_offsets.py -m gpu
Measured there: 22 passed in 3.1 s; the slowest item is the world's fixture (0.4 s of host models), the slowest test call
test_row_families at 0.06 s.  tests/test_gpu_scan_matrix.py with the placed rows: 394 passed in 32 s (99 in 16 s before them).

Checked to bite, without faulting anything: memory-safe changes to scratch builds (never committed), each of which cuts an offset to its
low 32 bits -- the address then lies in the zeroed low part of the same buffer, which is why the buffer is one allocation from 0.
Build 1, all three in one library, run once over this module and tests/test_gpu_scan_matrix.py:
  kmp_regex.hip       text = arena + (uint32_t)pkt_off[k]
  kmp_relations.hip   off = (uint32_t)pkt_off[k]
  kmp_scan_stream_kernels.inc, packed kernel, `DEPTH == 3 && NT && !EMIT && !KMP_WHOLE`: off_first = plan[gw].off & 0xFFFFFFFF
13 failed, 403 passed.  Failed: test_row_families, test_flows_and_seams and test_load_selected at split, edge and behind (relation rows
empty from the first high payload on: 148, 130 and 308 wrong bits; the rules that name a relation or an expression, their flows and
their selection with them); test_row_placed[kmp_scan_packed_kernel<3, true, false>] at split, edge and behind (e.g. 261 of 3084, 351 of
3084, 0 of 3084) and test_trace_names_every_row_behind, whose child reports that row.  Every `low` case, every other placed row, the
counting variants, the emitters, the gapped arena and the refusals passed.
Build 2, the kmp_regex.hip change alone (in build 1 the relations are compared first), run once over this module: 9 failed, 13 passed --
the same nine tests, test_row_families now at the expressions' rows (850, 788 and 1642 wrong bits).
The rest of the GPU suite (874 tests outside these two modules) was not run against either build; none of its tests hands an arena
above 4 GiB to one of these three kernels, where alone the changes differ from the code as it is.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import (B32, PLACEMENTS, SPLIT_FRONT, VARIANTS, attach_placed, big_buffer, check_fold, check_offsets, check_packets,  # noqa: E402,F401
                         gm, meta_of_flows, placed_base, reset, slot_offsets, zero_slots)  # (torch first; big_buffer, gm: fixtures)

import bytetest_model as BM  # noqa: E402
import chain_model as CM  # noqa: E402
import flow_model as FM  # noqa: E402
import header_model as HM  # noqa: E402
import match_model as MM  # noqa: E402
import prep_model as PM  # noqa: E402
import regex_model as RM  # noqa: E402
import seam_model as SM  # noqa: E402
from regex_model import rx  # noqa: E402
from multithreading_string_matching_amd._lib import KmpGpuError  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_GENERAL, MODE_AUTOMATON, MODE_FILTER, OPT_FUSED, OPT_KERNEL, OPT_MODE, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher)
N, SPLIT_K, EDGE_K = 600, 293, 310
LENS = [0, 1, 15, 16, 17, 48, 300, 1500, 9000]
ALPHA = b"\n\n  0189aAbBxX=:/"
REACH = 98
JUNCTION = b"GET" + b"x9:" + b"HoSt" + b"key="         # from byte 40 on: GET 40..42, HoSt 46..49, key= 50..53
assert 40 + JUNCTION.index(b"HoSt") == SPLIT_FRONT - 2
NOCASE = [False, True, False, True, False]
WINDOWS = [(0, None), (0, None), (2, 400), (0, None), (0, None)]
RELATIONS = [(0, 2, 0, 10), (1, 2, 0, 4), (3, 1, None, None)]           # GET .. key=; host (nocase) .. key=; a natural one
CHAINS = [(0, (1, 0, 5), (2, 0, 5)), (3, (3, 0, 50))]                   # GET, host (nocase), key=; a natural one
HEADS = [HM.header(sport=(1000, 1003)), HM.header(length=(16, 300)), HM.header(length=(1500, 9000))]
TESTS = [BM.bt(4, BM.EQ, 0x486F5374, 46), BM.bt(4, BM.EQ, 0x74536F48, 46, little=True),      # "HoSt" at bytes 46..49, both byte orders
         BM.bt(2, BM.EQ, 0x6B65, 7, anchor=0),                          # "ke" 7 bytes behind a GET
         BM.bt(1, BM.GE, 0x41, 0), BM.isdataat(15), BM.bt(2, BM.GT, 0x3000, 1, anchor=1)]
EXPRS = [b"[0-9]$",
         rx(b"[aA]=", gate=0),
         rx(b"host.{2,12}$", nocase=True),             # from the junction's HoSt to a text end at byte 60
         rx(b"^.{46}..[sS]", dotall=True),             # bytes 0 .. 48
         rx(b"\\d{3,}", gate=2),
         rx(b"x[^a]", nocase=True),
         rx(b"^.{14}[aAbB]", dotall=True, gate=1),
         b"=a?b"]
N_PAT, R0, C0, H0, B0, X0 = 5, 5, 8, 10, 13, 19
RULES = [([0, X0 + 1], []), ([R0 + 0], [H0 + 0]), ([C0 + 0], []), ([B0 + 0, B0 + 1], []), ([B0 + 2], [X0 + 0]), ([X0 + 2], []),
         ([X0 + 3], [4]), ([H0 + 1, 3], [R0 + 2]), ([4], []), ([], [X0 + 5, 1]), ([C0 + 1], [B0 + 3]), ([H0 + 2, X0 + 4], [R0 + 1])]
P99_RULE = 8
FAMILIES = ("patterns", "relations", "chains", "headers", "bytetests", "regexes", "rules")


class World:
    def __init__(self, oracle):
        rng = np.random.default_rng(4032)
        alpha = np.frombuffer(ALPHA, dtype=np.uint8)
        self.p99 = bytes(rng.choice(alpha[alpha != 0x0A], REACH + 1).tobytes())
        self.pats = [b"GET", b"host", b"key=", b"aB", self.p99]
        lens = rng.choice(LENS, N)
        lens[:len(LENS)] = LENS
        flow = np.arange(N) // 5 % 40
        self.meta = meta = meta_of_flows(flow, seed=3)
        self.fo = fo = FM.flow_of_np(meta)
        assert np.array_equal(fo, FM.flow_of(meta))
        pr = SM.pred(fo, SM.direction(meta, fo))
        self.next_k = nxt = int(np.flatnonzero(pr == SPLIT_K)[0])
        assert nxt > SPLIT_K and nxt not in (EDGE_K - 1, EDGE_K)
        lens[SPLIT_K], lens[nxt], lens[EDGE_K - 1], lens[EDGE_K] = 1500, 300, 17, 300
        pay = []
        for k in range(N):
            L = int(lens[k])
            b = bytearray(rng.choice(alpha, L).tobytes())
            if k % 4 != 1:                                             # (the 0x00 bytes of tests/test_gpu_regex.py::_capture)
                for z in np.flatnonzero(rng.integers(0, 40, L) == 0):
                    b[int(z)] = 0
                if L >= 17 and k % 3 == 0:
                    b[13 if k % 2 else 16] = 0
            if L >= 15:
                for _ in range(1 + L // 300):
                    word = [b"GET", b"host", b"HoSt", b"key=", b"key="][int(rng.integers(5))]
                    at = int(rng.integers(0, L - len(word)))
                    b[at:at + len(word)] = word
            if L >= 300 and k % 7 == 2 and fo[k] != fo[SPLIT_K]:       # the 99-byte pattern inside a payload, in front of every 0x00
                b[:200] = bytes(b[:200]).replace(b"\0", b" ")
                b[100:100 + len(self.p99)] = self.p99
            if L >= 300 and k % 5 == 3:                                # the junction, and for every second one a text end at byte 60
                b[:64] = bytes(b[:64]).replace(b"\0", b":")
                b[40:40 + len(JUNCTION)] = JUNCTION
                if k % 2:
                    b[54:61] = b"018901\0"
            pay.append(b)
        assert SPLIT_K % 5 == 3 and SPLIT_K % 2 and SPLIT_K % 4 == 1
        # the seam: the pattern's first 60 bytes end SPLIT_K, the other 39 begin the next payload of its flow direction
        pay[SPLIT_K][-60:] = self.p99[:60]
        pay[nxt][:98] = bytes(pay[nxt][:98]).replace(b"\0", b" ")
        pay[nxt][:39] = self.p99[60:]
        assert 0 not in pay[SPLIT_K][-REACH:]
        self.payloads = [bytes(b) for b in pay]
        self.lens = [len(t) for t in self.payloads]
        self.slots = zero_slots(self.payloads)
        self.off, self.end = slot_offsets(self.slots)
        self.arena = np.frombuffer(b"".join(self.slots), dtype=np.uint8)
        self.k_of = {"split": SPLIT_K, "edge": EDGE_K}
        self.st, self.mat, self.rows, self.counts = {}, {}, {}, {}
        hrows = HM.header_rows(meta, self.lens, HEADS)
        for whole in (False, True):
            st = MM.starts(self.payloads, self.pats, WINDOWS, NOCASE, whole)
            hits = MM.hits(st, N_PAT)
            fam = {"patterns": hits, "relations": MM.relation_rows(st, self.pats, RELATIONS), "chains": CM.chain_rows(st, self.pats, CHAINS),
                   "headers": hrows, "bytetests": BM.bytetest_rows(self.payloads, self.pats, TESTS, WINDOWS, NOCASE, whole, st),
                   "regexes": RM.regex_rows(self.payloads, EXPRS, whole, hits)}
            mat = np.concatenate([fam[f] for f in FAMILIES[:-1]])
            assert mat.shape == (X0 + len(EXPRS), N)
            fam["rules"] = MM.rule_rows(mat, RULES)
            self.st[whole], self.mat[whole], self.rows[whole] = st, mat, fam
            self.counts[whole] = MM.oracle_counts(oracle, self.payloads, self.pats, NOCASE, whole)
        self.facts()

    def base(self, placement):
        return placed_base(placement, self.payloads, None, self.k_of.get(placement))

    def facts(self):
        s, t = SPLIT_K, self.payloads[SPLIT_K]
        st = self.st[False][s]
        # a payload on each side of 2^32 under every placed case, and 2^32 inside SPLIT_K at byte 48
        assert self.base("split") + int(self.off[s]) + SPLIT_FRONT == B32 and self.base("edge") + int(self.off[EDGE_K]) == B32
        assert int(self.off[EDGE_K - 1]) + 32 == int(self.off[EDGE_K]) and self.base("behind") > B32
        # what is planted around byte 48 of SPLIT_K, under the default text-end rule: the text ends at byte 60
        assert MM.text_end(t) == 60 and t[40:54] == JUNCTION
        assert 46 in st[1] and 40 in st[0] and 50 in st[2]                                  # host across 2^32; GET in front, key= behind
        fam = self.rows[False]
        assert fam["relations"][0, s] and fam["relations"][1, s] and MM.pair_exists([40], [50], 3, 0, 10) and MM.pair_exists([46], [50], 4, 0, 4)
        assert fam["chains"][0, s] and CM.chain_holds([[40], [46], [50], [], []], self.pats, CHAINS[0])
        assert BM.field(t, 60, 46, 4, False) == 0x486F5374 and BM.field(t, 60, 46, 4, True) == 0x74536F48 and fam["bytetests"][:3, s].all()
        m = RM.compiled(b"host.{2,12}$", nocase=True).search(t[:60])
        assert m and m.start() == 46 and m.end() == 60 and fam["regexes"][2, s]
        m = RM.compiled(b"^.{46}..[sS]", dotall=True).search(t[:60])
        assert m and m.end() == SPLIT_FRONT + 1 and fam["regexes"][3, s]
        for whole in (False, True):
            fam = self.rows[whole]
            for f in FAMILIES:                         # SPLIT_K is in a row of every family
                assert fam[f][:, s].any(), (f, whole)
            # every row of every family has a set and an unset bit on either side, of SPLIT_K and of EDGE_K
            for f in FAMILIES:
                for q, row in enumerate(fam[f]):
                    for lo, hi in ((slice(0, s), slice(s + 1, N)), (slice(0, EDGE_K), slice(EDGE_K, N))):
                        for part in (row[lo], row[hi]):
                            assert 0 < part.sum() < part.size, (f, q, whole, int(part.sum()), part.size)
        # the seam
        recs = self.recs = SM.records(self.meta, self.lens, REACH)
        j = int(np.flatnonzero(recs["next"] == self.next_k)[0])
        assert int(recs["prev"][j]) == s and int(recs["tail_len"][j]) == REACH
        self.seams = SM.payloads(self.payloads, recs)
        assert self.seams[j].find(self.p99) == REACH - 60 and all(self.p99 not in self.payloads[k] for k in np.flatnonzero(self.fo == self.fo[s]))
        assert self.rows[False]["rules"][:, s].any()   # SPLIT_K is among the payloads load_selected takes


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


@pytest.fixture(scope="module")
def sm():
    """the second context: the seams"""
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def dst():
    """the third context: the selection"""
    m = GpuMatcher(0)
    yield m
    m.close()


def setup(gm, world, placement, buf, whole=False):
    reset(gm)
    gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
    gm.set_patterns(world.pats, nocase=NOCASE)
    keep = attach_placed(gm, world.payloads, None, world.base(placement), buf)
    gm.set_windows(WINDOWS)
    gm.set_relations(RELATIONS)
    gm.set_chains(CHAINS)
    gm.set_meta(world.meta)
    gm.set_headers(HEADS)
    gm.set_bytetests(TESTS)
    gm.set_regexes(EXPRS)
    assert [gm.rel(0), gm.chain(0), gm.hdr(0), gm.btest(0), gm.regex(0)] == [R0, C0, H0, B0, X0]
    gm.set_rules(RULES)
    return keep


def check_family(res, rows, key, counts):
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, (key, [(int(q), int(k), bool(rows[q, k])) for q, k in bad[:8]])
    assert res[key].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    assert res["counts"].tolist() == list(counts)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_scan_counts_on_every_kernel_family(gm, world, big_buffer, placement):
    """kmpgpu_scan under gpu_support.VARIANTS (flat is not applicable to these lengths and runs what the dispatch puts in its place), both
    text-end rules; and kmpgpu_effective_bytes"""
    try:
        keep = setup(gm, world, placement, big_buffer)
        for whole in (False, True):
            gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
            for name, mode, kernel, fused in VARIANTS:
                gm.set_option(OPT_MODE, mode); gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
                assert gm.scan()[0].tolist() == world.counts[whole], (placement, name, whole)
        assert gm.effective_bytes() == PM.effective_bytes(world.arena, world.off, world.lens)
        assert gm.arena_info() == (N, sum(world.lens))
        del keep
    finally:
        reset(gm)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_hits_and_offsets(gm, world, big_buffer, placement):
    """kmpgpu_scan_packets and kmpgpu_scan_offsets: every (payload, offset, pattern) triple, under the windows"""
    try:
        for whole in (False, True):
            keep = setup(gm, world, placement, big_buffer, whole)
            check_packets(gm, world.rows[whole]["patterns"], world.counts[whole])
            check_offsets(gm, MM.records(world.st[whole]), world.counts[whole])
            del keep
    finally:
        reset(gm)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_row_families(gm, world, big_buffer, placement):
    """relations, chains, byte tests, expressions and rules, and the alert list of the rules"""
    try:
        for whole in (False, True):
            keep = setup(gm, world, placement, big_buffer, whole)
            fam, counts = world.rows[whole], world.counts[whole]
            check_family(gm.scan_relations(hits=True), fam["relations"], "rel_pkt_counts", counts)
            check_family(gm.scan_chains(hits=True), fam["chains"], "chain_pkt_counts", counts)
            check_family(gm.scan_headers(hits=True), fam["headers"], "hdr_pkt_counts", counts)
            check_family(gm.scan_bytetests(hits=True), fam["bytetests"], "bt_pkt_counts", counts)
            check_family(gm.scan_regexes(hits=True), fam["regexes"], "rx_pkt_counts", counts)
            check_family(gm.scan_rules(hits=True), fam["rules"], "rule_pkt_counts", counts)
            al = gm.scan_alerts("rules")
            assert [(int(a["packet"]), int(a["index"])) for a in al["alerts"]] == sorted((int(k), int(r)) for r, k in np.argwhere(fam["rules"]))
            assert al["n_found"] == int(fam["rules"].sum()) and al["n_packets"] == int(fam["rules"].any(axis=0).sum())
            del keep
    finally:
        reset(gm)


def check_seams(sm, world):
    """the seam records, and the seam arena byte for byte (the download is of the small seam arena)"""
    want, off, ln = SM.arena(world.seams)
    assert sm.seams().tobytes() == world.recs.tobytes()
    assert sm.arena_info() == (len(world.seams), sum(len(s) for s in world.seams))
    a, o, l = sm.arena_download()
    assert np.array_equal(o, off) and np.array_equal(l, ln)
    assert len(a) >= len(want) and not a[len(want):].any()
    bad = np.flatnonzero(a[:len(want)] != want)
    assert bad.size == 0, [(int(b), int(np.searchsorted(off, b, side="right")) - 1) for b in bad[:8]]
    assert sm.meta().tobytes() == world.meta[world.recs["next"].astype(np.int64)].tobytes()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_flows_and_seams(gm, sm, world, big_buffer, placement):
    """kmpgpu_flows_build and the rules per flow; kmpgpu_load_seams reading the high source, and the rules with the seams' pattern rows"""
    fo, n_flows = world.fo, int(world.fo.max()) + 1
    try:
        keep = setup(gm, world, placement, big_buffer)
        reset(sm)
        sm.set_patterns(world.pats, nocase=NOCASE)
        mat, counts = world.mat[False], world.counts[False]
        assert gm.build_flows() == n_flows
        plain = FM.flow_rules(mat, fo, RULES, n_flows)
        assert 0 < plain.sum() < plain.size
        check_fold(gm, "rules", "flow", plain, counts)
        assert sm.load_seams(gm, REACH) == len(world.recs)
        check_seams(sm, world)
        seam_hits = MM.hits(MM.starts(world.seams, world.pats, None, NOCASE, False), N_PAT)
        want = SM.flow_rules(mat, seam_hits, fo, fo[world.recs["next"].astype(np.int64)], RULES, n_flows)
        f = int(fo[SPLIT_K])
        assert want[P99_RULE, f] and not plain[P99_RULE, f]          # the 99 bytes across the seam behind SPLIT_K, and nowhere else in its flow
        res = gm.scan_flow_seams(sm, hits=True)
        bad = np.argwhere(res["hits"] != want)
        assert bad.size == 0, [(int(r), int(x), bool(want[r, x])) for r, x in bad[:8]]
        assert res["flow_counts"].tolist() == want.sum(axis=1).tolist() and res["any"].tolist() == want.any(axis=0).tolist()
        assert res["counts"].tolist() == counts
        del keep
    finally:
        reset(gm, sm)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_load_selected(gm, dst, world, oracle, big_buffer, placement):
    """kmpgpu_load_selected of the rules' any[] out of the high source: arena, index and metadata, then a scan of the selection"""
    try:
        keep = setup(gm, world, placement, big_buffer)
        reset(dst)
        dst.set_patterns(world.pats, nocase=NOCASE)
        sel = world.rows[False]["rules"].any(axis=0)
        assert sel[SPLIT_K] and 0 < sel[:SPLIT_K].sum() < SPLIT_K and 0 < sel[SPLIT_K + 1:].sum() < N - SPLIT_K - 1
        res = gm.scan_rules()
        assert res["any"].tolist() == sel.tolist()
        idx = dst.load_selected(gm, res["any"]).astype(np.int64)
        assert idx.tolist() == np.flatnonzero(sel).tolist()
        ln = np.asarray(world.lens, dtype=np.uint32)[idx]
        want_off, want_arena = PM.gather_slots(world.arena, world.off[idx], ln)
        a, off, l = dst.arena_download()
        assert np.array_equal(off, want_off) and np.array_equal(l, ln)
        assert len(a) == len(want_arena) + 64 and np.array_equal(a[:len(want_arena)], want_arena) and not a[len(want_arena):].any()
        assert dst.meta().tobytes() == world.meta[idx].tobytes()
        mine = [world.payloads[int(k)] for k in idx]
        check_packets(dst, MM.hits(MM.starts(mine, world.pats, None, NOCASE), N_PAT), MM.oracle_counts(oracle, mine, world.pats, NOCASE))
        del keep
    finally:
        reset(gm, dst)


def test_gapped_low_and_high(gm, world, big_buffer):
    """The payloads with even k in the first MiB of the buffer and the odd ones behind 2^32, index order k: not packed.  In place
    (KMPGPU_OPT_REPACK = 0) a wavefront of the general kernel goes from a low payload to a high one, and the nocase patterns ask
    kmp_slot_end_kernel for the furthest slot and the fold for everything up to it; repacked, the gather reads from both halves."""
    size = np.array([len(s) for s in world.slots], dtype=np.int64)
    off = np.zeros(N, dtype=np.int64)
    for par, start in ((0, 0), (1, B32 + 4096)):
        off[par::2] = start + np.cumsum(size[par::2]) - size[par::2]
    assert off[0::2].max() + 9008 < (1 << 20) and off[1::2].min() > B32 and not np.array_equal(np.sort(off), off)
    try:
        reset(gm)
        gm.set_option(OPT_REPACK, 0)
        gm.set_patterns(world.pats, nocase=NOCASE)
        keep = attach_placed(gm, world.payloads, None, 0, big_buffer, off=off)
        for mode in (MODE_FILTER, MODE_AUTOMATON):
            gm.set_option(OPT_MODE, mode); gm.set_option(OPT_KERNEL, KERNEL_GENERAL); gm.set_option(OPT_FUSED, 0)
            assert gm.scan()[0].tolist() == world.counts[False], mode
        reset(gm)
        gm.set_option(OPT_REPACK, 1)
        keep = attach_placed(gm, world.payloads, None, 0, big_buffer, off=off)
        gm.set_windows(WINDOWS)
        check_packets(gm, world.rows[False]["patterns"], world.counts[False])
        a, o, l = gm.arena_download()                  # the packed copy, which is small
        assert np.array_equal(o, world.off.astype(np.uint64)) and l.tolist() == world.lens
        assert len(a) == world.end + 64 and np.array_equal(a[:world.end], world.arena) and not a[world.end:].any()
        del keep
    finally:
        reset(gm)


def test_an_index_that_leaves_the_arena_is_refused(gm, world, big_buffer):
    """kmp_validate_index_kernel's compare in 64 bits: arena_bytes one slot short of the last high slot's end is refused, the exact end is
    taken"""
    base = world.base("behind")
    try:
        reset(gm)
        gm.set_patterns(world.pats, nocase=NOCASE)
        keep = attach_placed(gm, world.payloads, None, base, big_buffer)
        assert gm.arena_info() == (N, sum(world.lens))
        for short in (16, 1):
            with pytest.raises(KmpGpuError, match="exceeds the arena"):
                gm.attach_arena(*keep, arena_bytes=base + world.end - short)
        with pytest.raises(KmpGpuError, match="exceeds the arena"):
            gm.attach_arena(*keep, arena_bytes=(base + world.end) & 0xFFFFFFFF)      # what a 32-bit compare would take for the end
        gm.attach_arena(*keep, arena_bytes=base + world.end)
        assert gm.scan()[0].tolist() == world.counts[False]
        del keep
    finally:
        reset(gm)
