"""The host model of matching: what every exact comparison of the GPU tests rests on.  numpy and bytes only, no GPU, nothing of the
library; tests/test_match_model.py holds it to the CPU oracle.

The rule, payload by payload: the text is t = payload[:E_k], E_k = the payload's first 0x00, or its end under OPT_WHOLE_PAYLOAD
(`whole`); for a nocase pattern text and pattern are folded (ASCII A-Z to a-z, every other byte as it is); every start of a pattern
is found by bytes.find from s + 1, overlapping starts included; the starts inside the pattern's window [first, last] are its
matches.  `starts` is that rule and the one primitive: records, hit matrices, counts, rule rows and relation rows are derived from
what it returns.  Relation (a, b, dmin, dmax) holds in a payload where some start sa of a and some start sb of b have
dmin <= sb - (sa + len(a)) <= dmax, looked for over all pairs.

The totals that kmpgpu_scan returns (every match, windows or not) come from the CPU oracle instead: oracle_counts.
"""
import numpy as np

U32_MAX = 0xFFFFFFFF
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
RULE_NOT = 0x80000000                                # KMPGPU_RULE_NOT: the term's row must not hold the payload
REMAP = 0xFF                                         # what oracle_counts writes over 0x00 under `whole`: in no pattern (asserted there)


def fold(x):
    """ASCII A-Z -> a-z, every other byte as it is (bytes / bytearray -> bytes, anything else -> a new uint8 array)"""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x).lower()                      # bytes.lower() touches ASCII A-Z only
    x = np.array(x, dtype=np.uint8, copy=True)
    x[(x >= 0x41) & (x <= 0x5A)] += 0x20
    return x


def text_end(t, whole=False):
    z = -1 if whole else t.find(b"\0")
    return len(t) if z < 0 else z


def starts(payloads, pats, windows=None, nocase=None, whole=False):
    """starts[k][i]: the in-window start offsets of pattern i in payload k, ascending.  windows: (first, last) per pattern, a last
    of None = 0xFFFFFFFF; None / []: the default for every pattern"""
    nocase = nocase or [False] * len(pats)
    assert not windows or len(windows) == len(pats)
    win = [(a, U32_MAX if b is None else b) for a, b in windows] if windows else [(0, U32_MAX)] * len(pats)
    spec = [(fold(p) if nc else p, bool(nc), first, last) for p, nc, (first, last) in zip(pats, nocase, win)]
    out = []
    for text in payloads:
        t = text[:text_end(text, whole)]
        tf = fold(t)
        row = []
        for p, nc, first, last in spec:
            src = tf if nc else t
            ss = []
            s = src.find(p)
            while s >= 0:
                if first <= s <= last:
                    ss.append(s)
                s = src.find(p, s + 1)
            row.append(ss)
        out.append(row)
    return out


def records(st):
    """{(payload, offset, pattern)}"""
    return {(k, s, i) for k, row in enumerate(st) for i, ss in enumerate(row) for s in ss}


def per_payload(st, n_pat=0):
    """int64[n_pat, n_pkts]: the matches of pattern i in payload k.  n_pat is read off the first payload's row; where there may be
    no payload at all, say it"""
    return np.array([[len(ss) for ss in row] for row in st], dtype=np.int64).reshape(len(st), len(st[0]) if st else n_pat).T


def hits(st, n_pat=0):
    """bool[n_pat, n_pkts]"""
    return per_payload(st, n_pat) > 0


def counts(st, n_pat=0):
    """matches per pattern"""
    return [int(x) for x in per_payload(st, n_pat).sum(axis=1)]


def rule_rows(mat, rules):
    """bool[n_rules, n_pkts] of the (all_of, none_of) rules over the rows of mat"""
    rows = np.ones((len(rules), mat.shape[1]), dtype=bool)
    for r, (pos, neg) in enumerate(rules):
        for i in pos:
            rows[r] &= mat[i]
        for i in neg:
            rows[r] &= ~mat[i]
    return rows


def pair_exists(sa, sb, m_a, dmin, dmax):
    """the definition, over all pairs; a bound of None: that side is open"""
    lo = I32_MIN if dmin is None else dmin
    hi = I32_MAX if dmax is None else dmax
    for x in sa:
        for y in sb:
            if lo <= y - (x + m_a) <= hi:
                return True
    return False


def relation_rows(st, pats, relations):
    """bool[n_rel, n_pkts]"""
    rows = np.zeros((len(relations), len(st)), dtype=bool)
    for k, row in enumerate(st):
        memo = {}
        for q, rel in enumerate(relations):
            a, b, dmin, dmax = rel
            if row[a] and row[b]:
                if rel not in memo:
                    memo[rel] = pair_exists(row[a], row[b], len(pats[a]), dmin, dmax)
                rows[q, k] = memo[rel]
    return rows


def words(bits):
    """bool[..., n] -> uint64[..., ceil(n / 64)], LSB first, the bits behind n as 0"""
    n = bits.shape[-1]
    W = (n + 63) // 64
    pad = np.zeros(bits.shape[:-1] + (W * 64 - n,), dtype=bool)
    return np.packbits(np.concatenate([bits, pad], axis=-1), axis=-1, bitorder="little").view(np.uint64)


def flat_rules(rules):
    """(rule_off uint32[n + 1], terms uint32[]) as kmpgpu_set_rules takes them"""
    off = np.zeros(len(rules) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(a) + len(b) for a, b in rules])
    terms = np.array([t for a, b in rules for t in list(a) + [i | RULE_NOT for i in b]] or [0], dtype=np.uint32)
    return off, terms


def triples(recs):
    """the library's offset records as sorted (payload, offset, pattern)"""
    return sorted((int(r["packet"]), int(r["offset"]), int(r["pattern"])) for r in recs)


def oracle_counts_arena(oracle, arena, off, ln, pats, nocase=None, whole=False, threads=0):
    """what kmpgpu_scan returns, from the CPU oracle (which implements the strlen rule) over an arena and its index: a nocase pattern
    on the folded arena with the folded pattern; under `whole` on the 0x00 bytes mapped to REMAP -- a window equal to a pattern that
    holds neither 0x00 nor REMAP holds neither byte, so the mapping neither makes nor destroys a match, and leaves no 0x00 to stop at.
    nocase: None, one bool for all patterns, or a flag per pattern"""
    nocase = [bool(nocase)] * len(pats) if nocase is None or isinstance(nocase, bool) else nocase
    if whole:
        assert all(REMAP not in p and 0 not in p for p in pats)
        arena = np.array(arena, dtype=np.uint8, copy=True)
        arena[arena == 0] = REMAP
    cs = oracle.count(arena, off, ln, pats, threads)[0]
    if not any(nocase):
        return [int(x) for x in cs]
    fo = oracle.count(fold(arena), off, ln, [fold(p) for p in pats], threads)[0]
    return [int(fo[i]) if nocase[i] else int(cs[i]) for i in range(len(pats))]


def oracle_counts(oracle, payloads, pats, nocase=None, whole=False, threads=0):
    """oracle_counts_arena over payloads laid out back to back"""
    ln = np.array([len(t) for t in payloads], dtype=np.uint32)
    off = np.zeros(len(payloads), dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(payloads) + b"\0", dtype=np.uint8)
    return oracle_counts_arena(oracle, arena, off, ln, pats, nocase, whole, threads)
