"""tests/threshold_model.py, the definition of the rate thresholds the GPU tests compare against, held to verdicts written by hand, and its
vectorised form held to the loop."""
import numpy as np

import threshold_model as TM

S = 1_000_000                 # a second, in the microseconds the command-line programs use


def alerts(base_row, ts, thresholds, **keys):
    base = np.array([base_row], dtype=bool)
    return TM.run(base, ts, thresholds, **keys)["alert"][0].astype(int).tolist()


def test_the_fifth_login_in_sixty_seconds_fires_and_in_sixty_one_does_not():
    thr = [(0, "by_src", "at_least", 5, 60 * S)]
    src = [7] * 5
    # hits at 0, 15, 30, 45 and 59.999999 s: the window of the fifth reaches back to (and holds) the first
    assert alerts([1] * 5, [0, 15 * S, 30 * S, 45 * S, 60 * S - 1], thr, src=src) == [0, 0, 0, 0, 1]
    # ... at 60 s sharp the first has left it: T[k] - T[j] < window is strict
    assert alerts([1] * 5, [0, 15 * S, 30 * S, 45 * S, 60 * S], thr, src=src) == [0, 0, 0, 0, 0]
    assert alerts([1] * 5, [0, 15 * S, 30 * S, 45 * S, 61 * S], thr, src=src) == [0, 0, 0, 0, 0]
    # from the fifth on every hit inside a full window fires: these are base hits, not issued alerts
    assert alerts([1] * 7, [0, 1, 2, 3, 4, 5, 6], thr, src=[7] * 7) == [0, 0, 0, 0, 1, 1, 1]
    # a payload of the tracker that does not hit counts nothing and fires nothing
    res = TM.run(np.array([[1, 1, 0, 1, 1, 1]], dtype=bool), [0, 1, 2, 3, 4, 5], thr, src=[7] * 6)
    assert res["alert"][0].astype(int).tolist() == [0, 0, 0, 0, 0, 1] and res["window_counts"][0].tolist() == [1, 2, 2, 3, 4, 5]


def test_at_most_one_fires_once_per_burst_and_rearms_after_a_quiet_window():
    thr = [(0, "by_rule", "at_most", 1, 60 * S)]
    ts = [0, 1 * S, 2 * S, 59 * S, 60 * S, 61 * S, 200 * S, 201 * S]
    # 60 s: the hit at 0 has left, but those at 1, 2 and 59 have not; 200 s: the window is empty again
    assert alerts([1] * 8, ts, thr) == [1, 0, 0, 0, 0, 0, 1, 0]
    assert alerts([1] * 4, [0, 60 * S, 120 * S, 180 * S], thr) == [1, 1, 1, 1]
    # at_most 2: the first two of a burst
    assert alerts([1] * 4, [0, 1, 2, 3], [(0, "by_rule", "at_most", 2, 60 * S)]) == [1, 1, 0, 0]


def test_exactly_fires_on_the_nth_hit_alone():
    assert alerts([1] * 5, [0, 1, 2, 3, 4], [(0, "by_rule", "exactly", 3, 100)]) == [0, 0, 1, 0, 0]
    # ... and again when the window has slid down to n
    assert alerts([1] * 5, [0, 1, 2, 3, 50], [(0, "by_rule", "exactly", 1, 10)]) == [1, 0, 0, 0, 1]


def test_equal_timestamps_count_in_capture_order():
    # of two payloads with equal T only the earlier one counts for the other; a payload counts itself
    res = TM.run(np.ones((1, 4), dtype=bool), [5, 5, 5, 5], [(0, "by_rule", "at_least", 3, 1)])
    assert res["window_counts"][0].tolist() == [1, 2, 3, 4] and res["alert"][0].astype(int).tolist() == [0, 0, 1, 1]


def test_a_timestamp_that_steps_back_is_the_running_maximum():
    # ts 100, 40, 105: T = 100, 100, 105 -- the second payload sits at 100, not at 40
    res = TM.run(np.ones((1, 3), dtype=bool), [100, 40, 105], [(0, "by_rule", "at_least", 3, 6)])
    assert res["window_counts"][0].tolist() == [1, 2, 3]
    # ... with its own time 40 the third would have seen it leave a window of 6 (105 - 40), and a window of 5 drops both
    assert TM.run(np.ones((1, 3), dtype=bool), [100, 40, 105], [(0, "by_rule", "at_least", 3, 5)])["window_counts"][0].tolist() == [1, 2, 1]


def test_all_counts_every_earlier_hit_of_the_tracker():
    ts = [0, 1 << 40, 1 << 63, (1 << 64) - 2]
    res = TM.run(np.ones((1, 4), dtype=bool), ts, [(0, "by_rule", "at_least", 4, None)])
    assert res["window_counts"][0].tolist() == [1, 2, 3, 4] and res["alert"][0].astype(int).tolist() == [0, 0, 0, 1]
    # the widest window there is drops the hit at 0 only from 2^64 - 2 on... which is not below 2^64 - 2
    assert TM.run(np.ones((1, 4), dtype=bool), ts, [(0, "by_rule", "at_least", 4, (1 << 64) - 2)])["window_counts"][0].tolist() == [1, 2, 3, 3]


def test_two_thresholds_on_one_rule_must_both_pass():
    # "from the 2nd hit per source on, but at most 3 a window over all": an AND
    thr = [(0, "by_src", "at_least", 2, 100), (0, "by_rule", "at_most", 3, 100)]
    src = [1, 2, 1, 2, 1, 2]
    assert alerts([1] * 6, [0, 1, 2, 3, 4, 5], thr, src=src) == [0, 0, 1, 0, 0, 0]
    # a rule without thresholds alerts where it hits
    base = np.array([[1, 1, 1], [1, 0, 1]], dtype=bool)
    res = TM.run(base, [0, 1, 2], [(0, "by_rule", "at_least", 3, 100)])
    assert res["alert"].astype(int).tolist() == [[0, 0, 1], [1, 0, 1]]


def test_two_trackers_never_share_a_count():
    thr = [(0, "by_dst", "at_least", 2, 100)]
    assert alerts([1] * 4, [0, 1, 2, 3], thr, dst=[1, 2, 3, 4]) == [0, 0, 0, 0]
    assert alerts([1] * 4, [0, 1, 2, 3], thr, dst=[1, 2, 2, 1]) == [0, 0, 1, 1]
    res = TM.run(np.ones((1, 5), dtype=bool), [0, 1, 2, 3, 4], [(0, "by_flow", "at_least", 1, None)], flow_of=[0, 1, 0, 1, 0])
    assert res["window_counts"][0].tolist() == [1, 1, 2, 2, 3]


def test_run_fast_is_run():
    rng = np.random.default_rng(11)
    for case in range(300):
        n = int(rng.integers(1, 40))
        n_rules = int(rng.integers(1, 4))
        base = rng.integers(0, 3, (n_rules, n)) > 0
        style = case % 4
        if style == 0:
            ts = np.cumsum(rng.integers(0, 4, n)).astype(np.uint64)
        elif style == 1:
            ts = rng.integers(0, 6, n).astype(np.uint64)                       # steps back
        elif style == 2:
            ts = (np.uint64((1 << 63) - 5) + np.cumsum(rng.integers(0, 4, n)).astype(np.uint64))
        else:
            ts = np.minimum(np.uint64((1 << 64) - 2), np.uint64((1 << 64) - 40) + rng.integers(0, 60, n).astype(np.uint64))
        keys = {"src": rng.integers(0, 3, n), "dst": rng.integers(0, 2, n) * (1 << 31), "flow_of": rng.integers(0, 4, n)}
        thr = []
        for _ in range(int(rng.integers(1, 5))):
            window = [None, 1, 2, 3, 7, 1 << 62][int(rng.integers(0, 6))]
            thr.append((int(rng.integers(0, n_rules)), TM.TRACKS[int(rng.integers(0, 4))], TM.TYPES[int(rng.integers(0, 3))],
                        int(rng.integers(1, 5)), window))
        slow, fast = TM.run(base, ts, thr, **keys), TM.run_fast(base, ts, thr, **keys)
        assert np.array_equal(slow["window_counts"], fast["window_counts"]), (case, thr)
        assert np.array_equal(slow["alert"], fast["alert"]), (case, thr)
