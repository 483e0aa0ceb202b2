"""The kernels that run BEHIND the marking pass or beside the index -- chains, relations, header predicates, the flows build, fold and
expand, the two metadata kernels -- past their grid sizes, against the host models the suite already has (tests/match_model.py,
chain_model.py, header_model.py, flow_model.py, prep_model.py).  Every comparison is exact; nothing is timed.

The models' Python loops are kept away from the large inputs.  Payload k of a periodic arena is CLASSES[k % P] with P = 37, coprime to 64
and to 1 024, so that every class meets every lane, word and tile position; the first and the last payload are written by hand.  The model
runs on the P + 2 texts and numpy indexing expands its rows.  The metadata of the header tests has a period of its own (53 records);
the flows come from tests/flow_model.py's flow_of_np / records_np, which tests/test_flow_model.py holds to the dict model.

Where every kernel's second code path starts, read off the launchers in csrc/:

  row  code                                              second path starts at                                crossed by
  S1   kmp_chains_kernel: item += step (grid cap         n_chains * W > PAIR_CAP (8 192 on 256 CUs)           test_chains_through_three_rounds
       cu_count * 8 blocks of 4 wavefronts, one
       (chain, word) each)
  S2   kmp_relations_kernel: the same shape and cap      n_rel * W > PAIR_CAP                                 test_relations_through_three_rounds
  S3   kmp_headers_kernel: tile += gridDim.y,            tiles of HDR_TILE predicates > gridDim.y;            test_header_tiles[y3] (gridDim.y 3, 4 tiles),
       gridDim.y = min(tiles, 64, max(1, 1024 / bx)),    gridDim.y is 1 from 262 145 payloads on              test_header_tiles[y1] (gridDim.y 1, 3 tiles)
       bx = ceil(stride / 4); the __syncthreads() that
       guards s_out against the write-out before
  S4   kmp_flows_fold_kernel: r += gridDim.y,            more than 64 rows, or more rows than 1024 / bx       test_fold_rows130 (rows 0, 64, 128 in one block, packet
       gridDim.y = min(n_rows, 64, max(1, 1024 / bx)),                                                        and flow scope), test_fold_rows[y2] (gridDim.y 2, 5 rows),
       bx = ceil(W / 4)                                                                                       [y1-zipf] and [y1-each] (gridDim.y 1, 3 rows)
  S5   flows build: kmp_scan_local_kernel /              > 262 144 payloads (256 tiles per round of the       test_flows_build (ROUND + 1 and N_BIG; one, each, runs, zipf),
       kmp_scan_totals_kernel through flow_ws(), and     totals kernel); ids above 65 535; tables above       test_keep_meta_past_the_extract_cap
       blk_cnt[k / KMP_SCAN_TILE] + loc_idx[k] in        2^16 slots
       kmp_flows_number_kernel
  S6   kmp_flows_assign_kernel, kmp_flows_expand_kernel, flow words above 4 096, n_flows in the hundreds of   test_flows_build[each] (528 609 flows, 8 260 flow words),
       the reduce over folded rows in flow space         thousands                                            test_fold_rows[y1-each]
  S7   kmp_meta_extract_kernel: grid-stride, cap         > 1 048 576 frames                                   test_keep_meta_past_the_extract_cap
       4 096 x 256
  S8   kmp_meta_select_kernel: grid-stride, cap          > 262 144 source payloads                            test_load_selected_with_metadata_past_the_select_cap
       1 024 x 256

The asserts below the constants hold every shape past its threshold for the CU count of the device at hand.

Checked to bite: with each of these memory-safe changes made to a scratch build, the tests named failed here and the other tests of this
module passed; the older GPU modules over the same kernels (test_gpu_chains, _relations, _headers, _flows, _select, _rules, _alerts)
passed unless said otherwise -- the loop of kmp_chains_kernel ending after a wavefront's first item (S1: test_chains_through_three_rounds);
that of kmp_relations_kernel likewise (S2: test_relations_through_three_rounds; also test_gpu_relations.py's test_row_edges[5000], which
has a second round); the tile loop of kmp_headers_kernel ending after a block's first tile (S3: both test_header_tiles); the row loop of
kmp_flows_fold_kernel ending after a block's first row (S4: test_fold_rows130 and all three test_fold_rows); blk_cnt not added in
kmp_flows_number_kernel (S5: every test_flows_build but the two of one flow, all three test_fold_rows and
test_keep_meta_past_the_extract_cap[udp] at their builds; any arena of more than one scan tile shows this one, so test_gpu_flows.py's
test_shapes[1025] and [2049], its captures and its command lines failed as well); kmp_flows_expand_kernel reading no flow word from
4 096 on (S6: both test_flows_build[each], at their kmpgpu_flows_select); kmp_meta_extract_kernel ending after a thread's first frame
(S7: both test_keep_meta_past_the_extract_cap); kmp_meta_select_kernel after a thread's first payload (S8:
test_load_selected_with_metadata_past_the_select_cap).  The barrier at the head of the tile loop of kmp_headers_kernel has no change of
its own: a thread's write-out of s_out lies in front of the barrier behind the next tile's copy of the predicates, and every write to
s_out lies behind that one.

Every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_rows_scale.py -m gpu
"""
import functools
import itertools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_support import ONES, check_fold, check_rules, gm, lib, load_frames, meta_of_flows, reset  # noqa: E402,F401  (torch first; gm, lib: fixtures)

import torch  # noqa: E402

import chain_model as CM  # noqa: E402
import flow_model as FM  # noqa: E402
import header_model as HM  # noqa: E402
import match_model as MM  # noqa: E402
import prep_model as PM  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd._lib import KmpGpuError  # noqa: E402
from multithreading_string_matching_amd.host import META_DTYPE, HostArena  # noqa: E402
from multithreading_string_matching_amd.matcher import FLOW_DTYPE, OPT_FLOW_SLOTS, OPT_KEEP_META, GpuMatcher  # noqa: E402
from test_gpu_chains import place  # noqa: E402
from test_gpu_headers import ADDR, PORTS, PROTOS  # noqa: E402

U32 = 0xFFFFFFFF
H = HM.header
TILE = 256 * 4                        # KMP_SCAN_TILE
ROUND = 256 * TILE                    # one round of kmp_scan_totals_kernel (kmp_prep.hip)
HDR_TILE = _lib.HDR_TILE              # predicates kmp_headers_kernel stages at a time
HDR_MAX_BY = FOLD_MAX_BY = 64         # HDR_MAX_BY (kmp_headers.hip), FLOW_FOLD_MAX_BY (kmp_flows.hip)
META_EXTRACT_ITEMS = 4096 * 256       # one grid-stride round of kmp_meta_extract_kernel (kmp_launch_meta_extract)
META_SELECT_ITEMS = 1024 * 256        # ... of kmp_meta_select_kernel (kmp_launch_meta_select)
# one grid-stride round of kmp_chains_kernel / kmp_relations_kernel: cu_count * 8 blocks of 4 wavefronts (kmpgpu.hip, enqueue_family).
# (Without a device the module is collected and never run: the count of an MI355X stands in.)
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
PAIR_CAP = CUS * 8 * 4
N_BIG = 2 * ROUND + 4321              # two rounds of the totals kernel and a ragged rest
P = 37                                # the period of the arenas
P_META = 53                           # the period of the header tests' metadata
N_PAIR = 4097                         # payloads of the pairing tests: W = 65
W_PAIR = (N_PAIR + 63) // 64
N_ROWS_PAIR = (2 * PAIR_CAP + W_PAIR - 1) // W_PAIR + 3     # chains, and relations: a third round of (row, word) items
N_HDR_Y3, HEADS_Y3 = 65537, 3 * HDR_TILE + 1
N_FOLD_ROWS, N_FOLD_Y2 = 301, 100_003


def hdr_grid(n_pkts, n_hdr):
    """(gridDim.y, tiles) of kmp_launch_headers"""
    stride = ((n_pkts + 63) // 64 + 1) & ~1
    tiles = (n_hdr + HDR_TILE - 1) // HDR_TILE
    return min(tiles, HDR_MAX_BY, max(1, 1024 // ((stride + 3) // 4))), tiles


def fold_grid_y(n_pkts, n_rows):
    """gridDim.y of kmp_launch_flows_fold"""
    return min(n_rows, FOLD_MAX_BY, max(1, 1024 // (((n_pkts + 63) // 64 + 3) // 4)))


assert all(np.gcd(p, 1024) == 1 for p in (P, P_META)) and np.gcd(P, P_META) == 1
assert N_BIG > 2 * ROUND and N_BIG % TILE and N_BIG % 64 and PM.ROUND_ITEMS == ROUND
assert N_ROWS_PAIR * W_PAIR > 2 * PAIR_CAP and (N_ROWS_PAIR - 3) * W_PAIR <= 2 * PAIR_CAP + W_PAIR              # S1, S2: a third round
assert hdr_grid(N_HDR_Y3, HEADS_Y3) == (3, 4) and HEADS_Y3 % HDR_TILE == 1                                       # S3 (a): block y = 0 takes tiles 0 and 3
assert hdr_grid(N_BIG, 2 * HDR_TILE + 1) == (1, 3)                                                               # S3 (b)
assert fold_grid_y(N_FOLD_ROWS, 130) == 64 and fold_grid_y(N_FOLD_Y2, 5) == 2 and fold_grid_y(N_BIG, 3) == 1     # S4
assert N_BIG > 2 * META_SELECT_ITEMS and (N_BIG + 63) // 64 > 4096                                               # S8; S6: flow words of `each`


# ------------------------------------------------------------------------------------------------
# periodic arenas
# ------------------------------------------------------------------------------------------------
class Periodic:
    """n payloads: payload k is classes[k % P], but the first and the last one, which are written by hand.  `kind` indexes `texts`, the
    classes and the two special payloads, so a model's rows over the texts become the arena's by numpy indexing."""

    def __init__(self, n, classes, first, last):
        assert len(classes) == P and n >= 2
        self.n, self.texts = n, list(classes) + [first, last]
        self.kind = np.arange(n) % P
        self.kind[0], self.kind[n - 1] = P, P + 1
        self.len = np.array([len(t) for t in self.texts], dtype=np.uint32)[self.kind]
        self.times = np.bincount(self.kind, minlength=P + 2)

    def payloads(self):
        return [self.texts[i] for i in self.kind]

    def slots16(self):
        """(arena, off, len): every payload in a 16-byte slot, built without a loop over the payloads"""
        table = np.zeros((P + 2, 16), dtype=np.uint8)
        for i, t in enumerate(self.texts):
            assert len(t) <= 16
            table[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        arena = np.concatenate([table[self.kind].reshape(-1), np.zeros(64, dtype=np.uint8)])
        return arena, np.arange(self.n, dtype=np.uint64) * np.uint64(16), self.len

    def expand(self, text_rows):
        """bool[rows, P + 2] over the texts -> bool[rows, n]"""
        return text_rows[:, self.kind]

    def starts(self, pats):
        return MM.starts(self.texts, pats)

    def counts(self, oracle, pats):
        """what kmpgpu_scan returns: the oracle's counts of every text, times how often the text is there"""
        per = np.array([MM.oracle_counts(oracle, [t], pats) for t in self.texts], dtype=np.int64)
        return [int(x) for x in self.times @ per]


SMALL_PATS = [b"GET", b"ab", b"xyz", b"Q", b"zz"]


def _small_classes():
    """P texts of 0 .. 16 bytes, every length among them, patterns planted in some, a 0x00 in a few"""
    rng = random.Random("small-classes")
    out = []
    for i in range(P):
        L = i % 17
        b = bytearray(rng.choice(b"abxyzGETQ") for _ in range(L))
        if i % 3 == 0:
            p = SMALL_PATS[(i // 3) % len(SMALL_PATS)]
            if len(p) <= L:
                s = rng.randrange(0, L - len(p) + 1)
                b[s:s + len(p)] = p
        if i % 5 == 4 and L:
            b[rng.randrange(L)] = 0
        out.append(bytes(b))
    return out


SMALL_CLASSES = _small_classes()
SMALL_LAST = b"xyz GETab Qzz"         # the last payload holds every pattern


class Small:
    """a periodic arena of n payloads in 16-byte slots with the model's hit rows of SMALL_PATS"""

    def __init__(self, n):
        self.p = Periodic(n, SMALL_CLASSES, b"", SMALL_LAST)
        self.n, self.len = n, self.p.len
        text_hits = MM.hits(self.p.starts(SMALL_PATS), len(SMALL_PATS))
        assert text_hits[:, P + 1].all() and not text_hits[:, P].any()
        assert all(0 < text_hits[i, :P].sum() < P for i in range(len(SMALL_PATS)))
        self.hits = self.p.expand(text_hits)
        self.arena = self.p.slots16()

    def load(self, m, n_pat=len(SMALL_PATS)):
        m.set_patterns(SMALL_PATS[:n_pat])
        m.load_arena(*self.arena)
        assert m.arena_info() == (self.n, int(self.len.sum(dtype=np.uint64)))

    def counts(self, oracle, n_pat=len(SMALL_PATS)):
        return self.p.counts(oracle, SMALL_PATS[:n_pat])


@functools.lru_cache(maxsize=None)
def small(n):
    return Small(n)


FAMILY = {"packets": ("kmpgpu_scan_packets", "pkt_counts"), "relations": ("kmpgpu_scan_relations", "rel_pkt_counts"),
          "chains": ("kmpgpu_scan_chains", "chain_pkt_counts"), "headers": ("kmpgpu_scan_headers", "hdr_pkt_counts")}


def check_family(m, family, rows, counts=None):
    """hits, the per-row payload counts, any[] and counts of a family's own call, then the raw words: the bits at n_pkts and above are 0"""
    fn, key = FAMILY[family]
    res = getattr(m, "scan_" + family)(hits=True)
    if not np.array_equal(res["hits"], rows):
        bad = np.argwhere(res["hits"] != rows)
        raise AssertionError((len(bad), [(int(r), int(k), bool(rows[r, k])) for r, k in bad[:8]]))
    assert res[key].tolist() == rows.sum(axis=1).tolist()
    assert np.array_equal(res["any"], rows.any(axis=0))
    if counts is not None:
        assert res["counts"].tolist() == list(counts)
    n_rows, n = rows.shape
    W = (n + 63) // 64
    rc, any_w, hit_w = np.full(n_rows, 7, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64), np.full((n_rows, W), ONES, dtype=np.uint64)
    _lib.gpu_check(getattr(m._g, fn)(m._ctx, rc.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data, None, None), fn)
    assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))
    assert rc.tolist() == rows.sum(axis=1).tolist()
    return res


# ------------------------------------------------------------------------------------------------
# 1. S1, S2: the pairing kernels through three grid-stride rounds
# ------------------------------------------------------------------------------------------------
A3, B3, C4 = b"EFX", b"GHY", b"EGGZ"          # no letter of the filler: a planted content starts where it was put and nowhere else
PAIR_PATS = [A3, B3, C4]
D1, D2 = 23, 11                               # the planted distances: A .. B apart by 0 .. D1 - 1, B .. C by 0 .. D2 - 1


def _pair_classes():
    """P texts of 44 .. 100 bytes.  Three in four hold A, B and C, the r-th of them with B r % D1 bytes behind A's end and C 5 r % D2 bytes
    behind B's; the others hold A alone, nothing, A and a B too far behind it, or C in front of A."""
    rng = random.Random("pair-classes")
    out, r = [], 0
    for i in range(P):
        if i % 4 == 3:
            items = [[(2, A3)], [], [(2, A3), (5 + D1 + 2, B3)], [(9, C4), (20, A3)]][(i // 4) % 4]
        else:
            d1, d2 = r % D1, (5 * r) % D2
            items = [(2, A3), (5 + d1, B3), (8 + d1 + d2, C4)]
            r += 1
        out.append(place(44 + (7 * i) % 57, items, rng=rng))
    assert r >= D1
    return out


PAIR_LAST = place(50, [(2, A3), (5 + 4, B3), (8 + 4 + 3, C4)])          # the last payload: d1 = 4, d2 = 3


def _chain(c):
    """chain c's bounds from c: the first link walks through the planted distances, the second is open or closed by turns (closed so that
    the text with d1 = a stays in)"""
    a, w = c % D1, (c // D1) % 3
    return (0, (1, a, a + w), (2, 0, None) if c % 2 == 0 else (2, 0, (5 * a) % D2 + (c // D1) % 2))


def _relation(q):
    if q % 3 == 2:
        b = (q // 3) % D2
        return (1, 2, b, b + (q // (3 * D2)) % 2)
    a, w = q % D1, (q // D1) % 3
    return (0, 1, a, a + w)


@pytest.fixture(scope="module")
def pair(oracle):
    p = Periodic(N_PAIR, _pair_classes(), b"", PAIR_LAST)
    return p, p.starts(PAIR_PATS), p.counts(oracle, PAIR_PATS)


def _check_pair_rows(rows, text_rows):
    """what makes a mix-up of (row, word) in a later round visible: neighbouring rows differ, the words of a row differ, and the rows of
    the second and of the third round hold set and clear bits"""
    assert rows.shape == (N_ROWS_PAIR, N_PAIR) and rows[:, N_PAIR - 1].any()
    assert (rows[1:] != rows[:-1]).any(axis=1).all()
    assert text_rows[:, :P].any(axis=1).all() and not text_rows[:, :P].all(axis=1).any()
    items = MM.words(rows).reshape(-1)                       # item = row * W + word, as the kernels number them
    assert len(items) == N_ROWS_PAIR * W_PAIR > 2 * PAIR_CAP
    for lo, hi in ((PAIR_CAP, 2 * PAIR_CAP), (2 * PAIR_CAP, len(items))):
        assert (items[lo:hi] != 0).any() and (items[lo:hi] != ONES).any() and len(set(items[lo:hi].tolist())) > 8


def test_chains_through_three_rounds(gm, pair):
    p, st, counts = pair
    chains = [_chain(c) for c in range(N_ROWS_PAIR)]
    text_rows = CM.chain_rows(st, PAIR_PATS, chains)
    rows = p.expand(text_rows)
    _check_pair_rows(rows, text_rows)
    try:
        reset(gm)
        gm.set_patterns(PAIR_PATS)
        gm.load_arena(HostArena.from_payloads(p.payloads()))
        gm.set_chains(chains)
        check_family(gm, "chains", rows, counts)
    finally:
        reset(gm)


def test_relations_through_three_rounds(gm, pair):
    p, st, counts = pair
    relations = [_relation(q) for q in range(N_ROWS_PAIR)]
    text_rows = MM.relation_rows(st, PAIR_PATS, relations)
    rows = p.expand(text_rows)
    _check_pair_rows(rows, text_rows)
    try:
        reset(gm)
        gm.set_patterns(PAIR_PATS)
        gm.load_arena(HostArena.from_payloads(p.payloads()))
        gm.set_relations(relations)
        check_family(gm, "relations", rows, counts)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. S3: header tiles
# ------------------------------------------------------------------------------------------------
MASKS = [0, U32, 0xFF000000, 0xFFFF0000]
DPORTS = [(0, 65535), (53, 80), (1024, 65535)]


def _meta_table():
    """P_META records over ADDR / PORTS / PROTOS: every (protocol, source) pair with destination ports of every range of DPORTS"""
    t = np.zeros(P_META, dtype=META_DTYPE)
    i = np.arange(P_META)
    t["proto"] = np.array(PROTOS)[i % 3]
    t["src_ip"] = np.array(ADDR, dtype=np.uint32)[(i // 3) % 4]
    t["dst_port"] = np.array(PORTS)[(i // 12) % 6]
    t["dst_ip"] = np.array(ADDR, dtype=np.uint32)[(i // 2 + 1) % 4]
    t["src_port"] = np.array(PORTS)[(5 * i + 1) % 6]
    return t


META_TABLE = _meta_table()


def periodic_meta(n):
    return META_TABLE[np.arange(n) % P_META]


def _predicate(q):
    """predicate q from q: q and q + HDR_TILE differ in their destination ports and in their least length"""
    return H(proto=[None, 6, 17, 1][q % 4], src=(ADDR[(q >> 2) % 4], MASKS[(q >> 4) % 4]), dport=DPORTS[(q >> 6) % 3], length=(q // HDR_TILE, U32),
             bidir=q % 5 == 0)


def header_rows(meta, lens, heads):
    """HM.header_rows.  On a large arena (lengths of period P, metadata of period P_META, the first and the last payload apart) over one joint
    period, expanded, and held to the model's own answer on 4 096 payloads drawn at random and on both ends."""
    n, period = len(lens), P * P_META
    if n <= 100_000:
        return HM.header_rows(meta, lens, heads)
    k = np.arange(period, 2 * period)
    rows = HM.header_rows(meta[k], lens[k], heads)[:, np.arange(n) % period]
    ends = np.array([0, n - 1])
    rows[:, ends] = HM.header_rows(meta[ends], lens[ends], heads)
    ks = np.concatenate([np.arange(130), np.arange(n - 130, n), np.random.default_rng(n).integers(0, n, 4096)])
    assert np.array_equal(rows[:, ks], HM.header_rows(meta[ks], lens[ks], heads))
    return rows


@pytest.mark.parametrize("n,n_hdr", [(N_HDR_Y3, HEADS_Y3), (N_BIG, 2 * HDR_TILE + 1)], ids=["y3", "y1"])
def test_header_tiles(gm, oracle, n, n_hdr):
    s = small(n)
    meta = periodic_meta(n)
    heads = [_predicate(q) for q in range(n_hdr)]
    rows = header_rows(meta, s.len, heads)
    assert rows.any(axis=1).all() and np.flatnonzero(rows.all(axis=1)).tolist() == [0, 4, 8, 12]      # (the four that ask for nothing)
    assert all((rows[q] != rows[q + HDR_TILE]).any() for q in range(n_hdr - HDR_TILE))        # the rows of two tiles are never the same
    counts = s.counts(oracle)
    n_pat, last = len(SMALL_PATS), n_hdr - 1
    try:
        reset(gm)
        s.load(gm)
        gm.set_meta(meta)
        gm.set_headers(heads)
        check_family(gm, "headers", rows, counts)
        # as rule terms: a predicate of the first tile and one of the last
        assert gm.hdr(3) == n_pat + 3 and last // HDR_TILE == hdr_grid(n, n_hdr)[1] - 1
        rules = [([gm.hdr(3), gm.hdr(last)], []), ([gm.hdr(1)], [gm.hdr(last)]), ([0], [gm.hdr(2)]), ([gm.hdr(last - 1)], [1, gm.hdr(5)])]
        gm.set_rules(rules)
        mat = np.concatenate([s.hits, rows])
        want = MM.rule_rows(mat, rules)
        assert want.any(axis=1).all() and not want.all(axis=1).any()
        check_rules(gm, mat, rules, counts)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 3. S5, S6: the flows build
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zipf_flows(n, n_keys=200_000, seed=3):
    """a flow number per payload: a few big flows and a long tail of small ones"""
    rng = np.random.default_rng(seed + n)
    p = 1.0 / (np.arange(n_keys) + 1.0) ** 0.9
    return rng.choice(n_keys, n, p=p / p.sum())


def flow_shape(shape, n):
    k = np.arange(n)
    return {"one": lambda: np.zeros(n, dtype=np.int64), "each": lambda: k, "runs": lambda: (k + 32) // 64, "zipf": lambda: zipf_flows(n)}[shape]()


def check_build(m, meta, lens, directed=False):
    got = m.build_flows(directed)
    fo, recs = FM.flows_np(meta, lens, directed)
    assert got == len(recs)
    ids = m.flow_ids()
    assert ids.dtype == np.uint32 and np.array_equal(ids, fo), np.flatnonzero(ids != fo)[:8]
    r = m.flows()
    assert r.dtype == FLOW_DTYPE and r.tobytes() == recs.tobytes(), np.flatnonzero(r != recs)[:4]
    return fo, recs


def check_select(m, fo, n_flows, seed):
    """kmpgpu_flows_select of a random flow bitmap: the payloads of the chosen flows, the bits at n_pkts and above 0"""
    chosen = np.random.default_rng(seed).random(n_flows) < 0.5
    chosen[n_flows - 1] = True
    want = FM.expand(chosen, fo)
    bits = MM.words(chosen)
    out = np.full((len(fo) + 63) // 64, ONES, dtype=np.uint64)
    _lib.gpu_check(m._g.kmpgpu_flows_select(m._ctx, bits.ctypes.data, 0, out.ctypes.data, None), "kmpgpu_flows_select")
    assert np.array_equal(out, MM.words(want))
    assert np.array_equal(m.select_flows(chosen), out)


@pytest.mark.parametrize("shape", ["one", "each", "runs", "zipf"])
@pytest.mark.parametrize("n", [ROUND + 1, N_BIG])
def test_flows_build(gm, n, shape):
    s = small(n)
    meta = meta_of_flows(flow_shape(shape, n), seed=n)
    slots = 1 << int(n).bit_length()                       # the smallest power of two above n
    assert slots // 2 <= n < slots and slots > 1 << 16
    try:
        reset(gm)
        s.load(gm)
        gm.set_meta(meta)
        fo, recs = check_build(gm, meta, s.len)
        first = recs["first_packet"].astype(np.int64)
        if shape == "one":
            assert len(recs) == 1 and int(recs["n_packets"][0]) == n and int(recs["last_packet"][0]) == n - 1
        else:
            # first payloads in every round of the totals kernel (but a last round of one payload)
            assert np.bincount(first // ROUND, minlength=(n + ROUND - 1) // ROUND)[:(n + ROUND - TILE) // ROUND].min() > 0
        if shape == "each":
            assert len(recs) == n and np.array_equal(fo, np.arange(n))
        if shape == "zipf":
            assert 65535 < len(recs) < n // 2 and int(recs["n_packets"].max()) > 1000          # ids past 16 bits; hot flows
        before = (gm.flow_ids().tobytes(), gm.flows().tobytes())
        check_select(gm, fo, len(recs), seed=n)
        # a table that is as full as the library lets it get
        gm.set_option(OPT_FLOW_SLOTS, slots)
        check_build(gm, meta, s.len)
        assert (gm.flow_ids().tobytes(), gm.flows().tobytes()) == before
        check_select(gm, fo, len(recs), seed=n + 1)
        if shape == "zipf":
            gm.set_option(OPT_FLOW_SLOTS, 0)
            assert len(check_build(gm, meta, s.len, directed=True)[1]) > len(recs)
        # a table of no more slots than payloads is refused before anything is launched
        gm.set_option(OPT_FLOW_SLOTS, slots // 2)
        with pytest.raises(KmpGpuError, match=r"\(-2\).*KMPGPU_OPT_FLOW_SLOTS"):
            gm.build_flows()
    finally:
        gm.set_option(OPT_FLOW_SLOTS, 0)
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 4. S4: the fold
# ------------------------------------------------------------------------------------------------
def test_fold_rows130(gm, oracle):
    """301 payloads, 130 patterns: gridDim.y = 64, and block y = 0 folds rows 0, 64 and 128"""
    n, n_flows = N_FOLD_ROWS, 40
    grams = [bytes(t) for m in (2, 3, 4) for t in itertools.product(b"abcd", repeat=m)]
    pats = grams[:16 + 64] + grams[16 + 64::5][:50]
    assert len(pats) == len(set(pats)) == 130
    p = Periodic(n, _pair_classes(), b"", b"abcdabcd" * 8)
    rng = np.random.default_rng(4)
    w = 1.0 / (np.arange(n_flows) + 1.0) ** 1.2
    flow = np.concatenate([np.arange(n_flows), rng.choice(n_flows, n - n_flows, p=w / w.sum())])
    meta = meta_of_flows(flow, seed=9)
    hits = p.expand(MM.hits(p.starts(pats), len(pats)))
    counts = p.counts(oracle, pats)
    assert all(0 < hits[r].sum() < n for r in (0, 64, 128, 129)) and len({hits[r].tobytes() for r in range(130)}) > 100
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(HostArena.from_payloads(p.payloads()))
        gm.set_meta(meta)
        fo, recs = check_build(gm, meta, p.len)
        assert np.array_equal(fo, flow)
        folded = FM.fold(hits, fo)
        assert all(0 < folded[r].sum() < n_flows for r in (64, 128, 129))
        check_fold(gm, "patterns", "packet", folded, counts)
        # per flow: all 130 term rows are folded, then the rules
        rules = [([64, 128], [129]), ([128, 129], []), ([17, 100], [64]), ([], [128]), ([64], []), ([129, 0], [70]), ([128], [])]
        gm.set_rules(rules)
        want = FM.flow_rules(hits, fo, rules)
        per_packet = FM.fold(MM.rule_rows(hits, rules), fo)
        assert want.any(axis=1).all() and not want.all(axis=1).any() and (want & ~per_packet).any() and (per_packet & ~want).any()
        check_fold(gm, "rules", "flow", want, counts)
        check_fold(gm, "rules", "packet", per_packet, counts)
    finally:
        reset(gm)


@pytest.mark.parametrize("n,n_pat,shape", [(N_FOLD_Y2, 5, "zipf"), (N_BIG, 3, "zipf"), (N_BIG, 3, "each")], ids=["y2", "y1-zipf", "y1-each"])
def test_fold_rows(gm, oracle, n, n_pat, shape):
    s = small(n)
    flow = zipf_flows(n, 20_000) if n < ROUND else flow_shape(shape, n)
    meta = meta_of_flows(flow, seed=n)
    hits = s.hits[:n_pat]
    try:
        reset(gm)
        s.load(gm, n_pat)
        gm.set_meta(meta)
        n_flows = gm.build_flows()
        fo = FM.flow_of_np(meta)
        assert n_flows == int(fo.max()) + 1 and np.array_equal(gm.flow_ids(), fo)
        folded = FM.fold(hits, fo, n_flows)
        assert all(0 < folded[r].sum() < n_flows for r in range(n_pat))
        assert shape != "each" or ((n_flows + 63) // 64 > 4096 and np.array_equal(folded, hits))
        check_fold(gm, "patterns", "packet", folded, s.counts(oracle, n_pat))
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. S7: KMPGPU_OPT_KEEP_META past one grid-stride round of the extraction's metadata kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_keep_meta_past_the_extract_cap(gm, lib, proto):
    poff, plen, _ = lib.rule[proto]
    recs = [HM.extract(f, len(f), proto) for f in lib.frames]
    assert [r is not None for r in recs] == (plen >= 0).tolist()         # the model accepts exactly what the oracle accepts
    assert all(r is None or (r[0], r[1]) == (int(poff[k]), int(plen[k])) for k, r in enumerate(recs))
    kind_meta = HM.meta_array([r[2] if r is not None else (0, 0, 0, 0, 0) for r in recs])
    n = META_EXTRACT_ITEMS + 1
    kind = PM.make_sequence("mixed", n, plen, seed=n + len(proto))
    good = np.flatnonzero(plen > 0)
    kind[n - 1] = good[len(good) // 2]                     # the one frame of the second round is accepted
    acc = kind[plen[kind] >= 0]
    want = kind_meta[acc]
    assert len(acc) > n // 5 and len(np.unique(want)) > 50
    try:
        reset(gm)
        gm.set_patterns(lib.tags[:4])
        gm.set_option(OPT_KEEP_META, 1)
        assert load_frames(gm, lib.blob, lib.boff[kind], lib.cap[kind], proto) == len(acc)
        got = gm.meta()
        assert got.dtype == META_DTYPE and got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
        fo, flows = check_build(gm, want, plen[acc])
        assert 50 < len(flows) < len(lib.frames)
    finally:
        gm.set_option(OPT_KEEP_META, 0)
        reset(gm)
        gm.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))      # gives the arena back


# ------------------------------------------------------------------------------------------------
# 6. S8: kmpgpu_load_selected hands the metadata on, past one grid-stride round of its kernel
# ------------------------------------------------------------------------------------------------
def test_load_selected_with_metadata_past_the_select_cap(gm):
    n = N_BIG
    s = small(n)
    meta = periodic_meta(n)
    heads = [H(proto=17), H(src=(ADDR[1], U32), dport=(53, 80), bidir=True), H(proto=6, length=(3, 9))]
    rows = header_rows(meta, s.len, heads)
    random_half = np.random.default_rng(8).random(n) < 0.5
    rounds = np.zeros(n, dtype=bool)
    rounds[[3, META_SELECT_ITEMS + 5, 2 * META_SELECT_ITEMS + 7, n - 1]] = True      # one payload of every grid-stride round, and the last
    try:
        reset(gm)
        s.load(gm)
        gm.set_meta(meta)
        with GpuMatcher(0) as dst:
            dst.set_patterns(SMALL_PATS)
            for select in (random_half, rounds):
                idx = dst.load_selected(gm, select)
                assert idx.tolist() == np.flatnonzero(select).tolist()
                assert dst.arena_info() == (int(select.sum()), int(s.len[select].sum(dtype=np.uint64)))
                got = dst.meta()
                assert got.tobytes() == meta[select].tobytes(), np.flatnonzero(got != meta[select])[:8]
                dst.set_headers(heads)
                sub = rows[:, select]
                assert sub.any()
                check_family(dst, "headers", sub)
        assert gm.meta().tobytes() == meta.tobytes()          # the source is not written
    finally:
        reset(gm)
