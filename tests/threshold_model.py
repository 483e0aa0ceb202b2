"""Rate thresholds (kmpgpu_set_thresholds / kmpgpu_scan_thresholds; include/kmpgpu.h) written from the definition alone.

A threshold is (rule, "by_rule" | "by_src" | "by_dst" | "by_flow", "at_least" | "at_most" | "exactly", count, window), as
GpuMatcher.set_thresholds takes them; window None: no window.  T[k] = max(ts[0 .. k]);
    n[q][k]     = #{ j <= k : tracker(q, j) == tracker(q, k), base[r][j], T[k] - T[j] < window }
    alert[r][k] = base[r][k] and every threshold of rule r passes on its n.

``run`` is the sequential loop: a dict from tracker to a deque of the times of its hits, old ones dropped from the left.  ``run_fast``
is the same answer from a stable sort, a prefix sum and numpy's searchsorted, for inputs too long for the loop.
"""
from collections import deque

import numpy as np

TRACKS, TYPES = ("by_rule", "by_src", "by_dst", "by_flow"), ("at_least", "at_most", "exactly")


def trackers(track, n, src=None, dst=None, flow_of=None):
    keys = {"by_rule": np.zeros(n, dtype=np.int64), "by_src": src, "by_dst": dst, "by_flow": flow_of}[track]
    assert keys is not None and len(keys) == n, track
    return [int(x) for x in keys]


def passes(kind, cnt, count):
    return cnt >= count if kind == "at_least" else cnt <= count if kind == "at_most" else cnt == count


def run(base, ts, thresholds, src=None, dst=None, flow_of=None):
    """base: bool[n_rules, n] (what scan_rules gives), ts: n unsigned 64-bit times, src / dst / flow_of: int[n] where a threshold tracks
    by them.  Returns ``alert`` bool[n_rules, n] and ``window_counts`` int[n_thr, n] (n[q][k] for every k)."""
    base = np.asarray(base, dtype=bool)
    n_rules, n = base.shape
    ts = [int(t) for t in ts]
    assert len(ts) == n and all(0 <= t < 1 << 64 for t in ts)
    T, top = [], 0
    for t in ts:
        top = max(top, t)
        T.append(top)
    alert = base.copy()
    counts = np.zeros((len(thresholds), n), dtype=np.int64)
    for q, (rule, track, kind, count, window) in enumerate(thresholds):
        assert track in TRACKS and kind in TYPES and count >= 1 and (window is None or window >= 1)
        key = trackers(track, n, src, dst, flow_of)
        seen = {}                                      # tracker -> the times of its hits still inside the window
        for k in range(n):
            d = seen.setdefault(key[k], deque())
            if base[rule, k]:
                d.append(T[k])
            while window is not None and d and T[k] - d[0] >= window:
                d.popleft()
            counts[q, k] = len(d)
            if not passes(kind, len(d), count):
                alert[rule, k] = False
    return {"alert": alert, "window_counts": counts}


def run_fast(base, ts, thresholds, src=None, dst=None, flow_of=None):
    base = np.asarray(base, dtype=bool)
    n_rules, n = base.shape
    T = np.maximum.accumulate(np.asarray(ts, dtype=np.uint64)) if n else np.zeros(0, np.uint64)
    alert = base.copy()
    counts = np.zeros((len(thresholds), n), dtype=np.int64)
    for q, (rule, track, kind, count, window) in enumerate(thresholds):
        keys = {"by_rule": np.zeros(n, dtype=np.int64), "by_src": src, "by_dst": dst, "by_flow": flow_of}[track]
        keys = np.asarray(keys, dtype=np.int64)
        order = np.argsort(keys, kind="stable")
        ks, Ts, hit = keys[order], T[order], base[rule][order].astype(np.int64)
        C = np.concatenate(([0], np.cumsum(hit)))      # C[i]: hits at the sorted positions below i
        start = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1]))) if n else np.zeros(0, np.int64)
        end = np.concatenate((start[1:], [n]))
        cnt = np.zeros(n, dtype=np.int64)
        for a, b in zip(start.tolist(), end.tolist()):
            t = Ts[a:b]
            if window is None:
                lo = np.full(b - a, a, dtype=np.int64)
            else:
                # the first position of the run with T[k] - T[j] < window, i.e. T[j] > T[k] - window (every position where T[k] < window)
                w = np.uint64(window)
                edge = np.where(t >= w, t - w, np.uint64(0))
                lo = a + np.where(t >= w, np.searchsorted(t, edge, side="right"), 0)
            cnt[a:b] = C[np.arange(a, b) + 1] - C[lo]
        counts[q, order] = cnt
        ok = cnt >= count if kind == "at_least" else cnt <= count if kind == "at_most" else cnt == count
        back = np.zeros(n, dtype=bool)
        back[order] = ok
        alert[rule] &= back
    return {"alert": alert, "window_counts": counts}
