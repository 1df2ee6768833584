"""Prophage regions from the per-window phage track (``postprocess/prophages.py:524-602`` ``segment``).

The reference fits ``ruptures.KernelCPD(kernel="linear", min_size=3, jump=1)`` to the track, predicts with the penalties
1 .. 9, lets ``kneed`` pick one of the partitions and keeps the segments whose mean exceeds ``sensitivity``.  Neither
package is a dependency here:

* :func:`change_points` - kernel change-point detection with the linear kernel and a penalty is penalised optimal
  partitioning under the cost ``sum x^2 - (sum x)^2 / length``; PELT is exact, so the O(n^2) dynamic programme over prefix
  sums finds a partition of the same total.  On exact cost ties the two may pick different partitions (unpinned).
* :mod:`jaeger_amd.knee` - the knee.
* everything behind the knee is the reference's own numpy / pandas lines, quirks included: the segment in front of the
  first breakpoint is never a range, a range's score is the mean of rows ``s .. e`` INCLUSIVE, the ``sorted(...)`` of the
  merge has no effect and touching ranges merge.
"""

from __future__ import annotations

import logging
import traceback

import numpy as np

from .knee import KneeLocator

logger = logging.getLogger("Jaeger")

MIN_SIZE = 3
PENALTIES = range(1, 10)


def change_points(x, pen: float, min_size: int = MIN_SIZE) -> list[int]:
    """Sorted segment ends (the last is ``len(x)``) of the partition of ``x`` into segments of at least ``min_size``
    samples that minimises sum cost(a, b) + pen (segments - 1), cost(a, b) = sum x^2 - (sum x)^2 / (b - a) over
    x[a:b], in float64.  Ties go to the earliest last change point."""
    x = np.asarray(x, np.float64).ravel()
    n = len(x)
    if n < 2 * min_size:
        return [n]
    s1 = np.concatenate(([0.0], np.cumsum(x)))
    s2 = np.concatenate(([0.0], np.cumsum(x * x)))
    best = np.full(n + 1, np.inf)
    best[0] = -float(pen)                                   # every segment pays pen, the first gets it back
    last = np.zeros(n + 1, np.int64)
    starts = np.arange(n + 1)
    for t in range(min_size, n + 1):
        a = starts[:t - min_size + 1]                       # segment x[a:t]; best[1 .. min_size - 1] stay infinite
        d = s1[t] - s1[a]
        total = best[a] + (s2[t] - s2[a]) - d * d / (t - a) + pen
        k = int(np.argmin(total))
        best[t], last[t] = total[k], k
    ends, t = [], n
    while t > 0:
        ends.append(t)
        t = int(last[t])
    return ends[::-1]


def merge_overlapping_ranges(intervals):
    """``postprocess/helpers.py:604-632``: merges in the given order (the reference's ``sorted`` result is dropped);
    a range that starts where the last one ends merges into it."""
    if len(intervals) == 0:
        return []
    merged = [intervals[0]]
    for current_start, current_end in intervals[1:]:
        last_start, last_end = merged[-1]
        if current_start <= last_end:
            merged[-1][1] = max(last_end, current_end)
        else:
            merged.append([current_start, current_end])
    return merged


class _Partitions:
    """What the reference holds as the fitted ``KernelCPD``: ``predict(pen=...)``."""

    def __init__(self, track):
        self.track = np.asarray(track, np.float64)
        self._memo = {}

    def predict(self, pen):
        if pen not in self._memo:
            self._memo[pen] = change_points(self.track, pen)
        return list(self._memo[pen])


def segment(logits_df: dict, cutoff_length: int = 500_000, sensitivity: float = 1.5, identifier: str = "phage",
            fit=_Partitions, knee_locator=KneeLocator) -> dict:
    """``logits_df``: contig -> [frame, host, length] (:func:`jaeger_amd.prophage_inputs.logits_to_df_v2`) ->
    contig -> [ranges (k, 2) in windows, their mean scores]; ``[[], []]`` where nothing is found or anything raises.
    ``fit`` / ``knee_locator`` stand where the reference has ruptures and kneed (tests replay recorded ones)."""
    phage_cordinates = {}
    for key, (tmp, host, length) in logits_df.items():
        if length <= cutoff_length:
            continue
        try:
            algo = fit(tmp[identifier].to_numpy())
            if bkpts := [algo.predict(pen=i) for i in PENALTIES if len(algo.predict(pen=i)) > 1]:
                bkpt_lens = np.array([len(b) for b in bkpts])
                kn = knee_locator(bkpt_lens, list(range(len(bkpts))), curve="convex", direction="decreasing")
                bkpt_index = ([len(b) for b in bkpts].index(kn.knee) if kn.knee else np.searchsorted(bkpt_lens, 1))
                if bkpt_index == len(bkpt_lens):
                    bkpt_index = None
                ranges = [bkpts[bkpt_index][i:i + 2] for i in range(len(bkpts[bkpt_index]) - 1)]
                range_scores = np.array([tmp.loc[s:e][identifier].mean() for s, e in ranges])
                range_mask = range_scores > sensitivity
                selected_ranges = merge_overlapping_ranges(np.array(ranges)[range_mask])
                selected_ranges = np.array(selected_ranges)
                phage_cordinates[key] = [selected_ranges, range_scores[range_mask]]
            else:
                phage_cordinates[key] = [[], []]
        except Exception:
            phage_cordinates[key] = [[], []]
            logger.debug(traceback.format_exc())
    return phage_cordinates
