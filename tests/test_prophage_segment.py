"""Prophage segmentation (``jaeger_amd.prophage_segment`` / ``jaeger_amd.knee``): the change-point dynamic programme
against exhaustive search, the knee against hand-computed curves, ``segment`` against the reference's own lines
(tests/golden/prophage_segment.json, made by tests/golden/make_golden_prophage_report.py)."""
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"


def _cost(x, a, b):
    s = x[a:b]
    return float((s * s).sum() - s.sum() ** 2 / (b - a))


def _all_partitions(n, min_size=3):
    """Every list of segment ends (last = n) with all segments >= min_size."""
    def rec(start):
        if n - start >= min_size:
            yield [n]
        for end in range(start + min_size, n - min_size + 1):
            for rest in rec(end):
                yield [end] + rest
    return list(rec(0))


def _total(x, ends, pen):
    starts = [0] + ends[:-1]
    return sum(_cost(x, a, b) for a, b in zip(starts, ends)) + pen * (len(ends) - 1)


@pytest.mark.parametrize("n", [6, 7, 9, 11, 12, 14])
def test_change_points_find_the_exhaustive_optimum(n):
    """Seeded float tracks, every penalty 1 .. 9: the partition's total equals the minimum over ALL partitions with
    segments of at least 3 samples (equality of totals to 1e-9 relative - the sums are taken in another order - and of the
    partition itself wherever the minimum is unique by more than that)."""
    from jaeger_amd.prophage_segment import change_points
    rng = np.random.Generator(np.random.PCG64(100 + n))
    parts = _all_partitions(n)
    assert [n] in parts and all(min(np.diff([0] + p)) >= 3 for p in parts)
    for trial in range(6):
        x = rng.normal(0, 1, n) * (1 + trial)
        x[rng.integers(0, n):] += rng.normal(0, 3)
        for pen in range(1, 10):
            got = change_points(x, pen)
            totals = np.array([_total(x, p, pen) for p in parts])
            best = float(totals.min())
            assert got in parts
            assert _total(x, got, pen) <= best + 1e-9 * max(1.0, abs(best))
            if np.sum(totals <= best + 1e-7 * max(1.0, abs(best))) == 1:
                assert got == parts[int(np.argmin(totals))]


def test_change_points_short_tracks_and_a_step():
    from jaeger_amd.prophage_segment import change_points
    for n in range(0, 6):
        assert change_points(np.arange(n, dtype=float) ** 2, 1) == [n]
    step = np.concatenate((np.zeros(10), np.full(7, 5.0), np.zeros(13)))
    for pen in range(1, 10):
        assert change_points(step, pen) == [10, 17, 30]              # each change saves 5^2 x (>= 3.9) >> 9
    assert change_points(step, 1e6) == [30]
    assert change_points(np.zeros(12), 1) == [12]


def test_knee_pins_the_restatement():
    """These pin the restatement as scipy and numpy behave here - not the kneed package, which is not installed."""
    from jaeger_amd.knee import KneeLocator, knee_convex_decreasing
    # hand-computed: x = 0 .. 4, y = 10, 4, 2, 1, 0.5 (convex, decreasing).  x_n = 0, .25, .5, .75, 1;
    # y_n = (y - .5) / 9.5 = 1, .368, .158, .053, 0 -> flipped 0, .632, .842, .947, 1; difference 0, .382, .342, .197, 0:
    # one maximum at index 1, threshold .382 - .25 = .132, and the difference first drops below it at index 4 -> x = 1
    assert knee_convex_decreasing([0, 1, 2, 3, 4], [10, 4, 2, 1, 0.5]) == 1
    assert KneeLocator([0, 1, 2, 3, 4], [10, 4, 2, 1, 0.5], curve="convex", direction="decreasing").knee == 1
    # a straight line has no interior extremum of the difference curve -> flat zero difference: every point is a
    # (non-strict) maximum, the walk starts at index 0 and the difference never drops below the threshold: no knee
    assert knee_convex_decreasing([0, 1, 2, 3], [3, 2, 1, 0]) is None
    # what the segmentation feeds it: non-increasing x with repeats (x_n starts at 1.0: the walk ends before it began)
    assert knee_convex_decreasing(np.array([8, 8, 6, 6, 6, 3, 3]), list(range(7))) is None
    # a single point (the scipy here interpolates it) and all-equal x: 0 / 0 -> NaN everywhere, no comparison with NaN is
    # true, argrelextrema finds NO maximum -> no knee
    from scipy.signal import argrelextrema
    assert argrelextrema(np.full(3, np.nan), np.greater_equal)[0].size == 0
    assert knee_convex_decreasing(np.array([5]), [0]) is None
    assert knee_convex_decreasing(np.array([4, 4, 4]), [0, 1, 2]) is None
    with pytest.raises(NotImplementedError):
        KneeLocator([0, 1], [1, 0], curve="concave", direction="increasing")


def _replay(case):
    class Fit:
        def __init__(self, track):
            pass

        def predict(self, pen):
            if case.get("raise_in_predict"):
                raise RuntimeError("replayed failure")
            return list(case["bkpts"][str(pen)])

    class Knee:
        def __init__(self, x, y, curve, direction):
            assert (curve, direction) == ("convex", "decreasing")
            assert list(x) == [len(case["bkpts"][str(p)]) for p in range(1, 10) if len(case["bkpts"][str(p)]) > 1]
            assert list(y) == list(range(len(x)))
            self.knee = case["knee"]

    return Fit, Knee


def test_segment_equals_the_reference_lines():
    """The reference's ``segment`` with recorded breakpoints and knees replayed into it (golden) against ours with the
    same replay: ranges as consecutive pairs (never the first segment), INCLUSIVE means, the merge of touching ranges, the
    fallback index without a knee, ``[[], []]`` from the except path, the skip at the cutoff."""
    from jaeger_amd.prophage_segment import segment
    gold = json.loads((GOLDEN / "prophage_segment.json").read_text())
    track = np.array(gold["track"])
    seen = set()
    for case in gold["cases"]:
        fit, knee = _replay(case)
        frame = pd.DataFrame({"phage": track.copy(), "bacteria": 1 - track})
        got = segment({"ctg": [frame, "bacteria", case["length"]]}, cutoff_length=case["cutoff"],
                      sensitivity=case["sensitivity"], identifier="phage", fit=fit, knee_locator=knee)
        if case["expected"] is None:
            assert got == {}, case["name"]
            continue
        ranges, scores = got["ctg"]
        assert np.asarray(ranges).tolist() == case["expected"]["ranges"], case["name"]
        assert [float(s) for s in np.asarray(scores).tolist()] == case["expected"]["scores"], case["name"]
        seen.add((len(case["expected"]["ranges"]), len(case["expected"]["scores"])))
    assert (2, 3) in seen and (0, 0) in seen          # the merge leaves more scores than ranges; the empty results


def test_segment_end_to_end_on_a_track_with_an_island():
    """Our own change points and knee, no replay: a high plateau over windows 120 .. 135 of 260 comes back as one range."""
    from jaeger_amd.prophage_segment import segment
    rng = np.random.Generator(np.random.PCG64(3))
    track = rng.normal(0.3, 0.05, 260)
    track[120:135] += 3.0
    got = segment({"c": [pd.DataFrame({"phage": track}), "bacteria", 520_000]}, cutoff_length=500_000, sensitivity=1.5)
    ranges, scores = got["c"]
    assert np.asarray(ranges).tolist() == [[120, 135]] and len(scores) == 1 and 2.8 < scores[0] < 3.5
