"""Knee of a convex, decreasing curve: Kneedle (Satopaa, Albrecht, Irwin, Raghavan 2011, "Finding a 'Kneedle' in a
Haystack") as ``kneed.KneeLocator(x, y, curve="convex", direction="decreasing")`` runs it with its defaults - ``S = 1``,
``interp_method="interp1d"``, offline (the first knee is returned).  The one caller is the choice among the change-point
partitions of a phage track (``postprocess/prophages.py:562-573``), whose ``x`` is a non-increasing list of breakpoint
counts with repeats.

The package is not a dependency: the steps below are written from the paper and the package's documented behaviour, both
scipy calls are the real ones, and degenerate inputs (a single point, all-equal ``x``) do whatever scipy and numpy do with
them - agreement with the package on those is unpinned.
"""

from __future__ import annotations

import numpy as np


def _normalize(a: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", divide="ignore"):       # all-equal input: NaN, as the package computes it
        return (a - a.min()) / (a.max() - a.min())


def knee_convex_decreasing(x, y, S: float = 1.0):
    """The knee's ``x`` value, or None."""
    from scipy.interpolate import interp1d
    from scipy.signal import argrelextrema
    x, y = np.array(x), np.array(y)
    ds_y = interp1d(x, y)(x)                                  # "smoothing": the interpolant evaluated at its own knots
    x_norm, y_norm = _normalize(x), _normalize(ds_y)
    y_norm = y_norm.max() - y_norm                            # convex + decreasing
    y_diff = y_norm - x_norm
    maxima = argrelextrema(y_diff, np.greater_equal)[0]
    minima = argrelextrema(y_diff, np.less_equal)[0]
    if not maxima.size:
        return None
    tmx = y_diff[maxima] - S * np.abs(np.diff(x_norm).mean())
    threshold, threshold_index, next_max = 0.0, 0, 0
    for i, xv in enumerate(x_norm):
        if i < maxima[0]:
            continue
        if xv == 1.0:
            break
        if (maxima == i).any():
            threshold, threshold_index = tmx[next_max], i
            next_max += 1
        if (minima == i).any():
            threshold = 0.0
        if y_diff[i + 1] < threshold:
            return x[threshold_index]
    return None


class KneeLocator:
    """The slice of ``kneed.KneeLocator`` the segmentation reads: ``.knee``."""

    def __init__(self, x, y, curve: str = "convex", direction: str = "decreasing", S: float = 1.0):
        if (curve, direction) != ("convex", "decreasing"):
            raise NotImplementedError(f"KneeLocator(curve={curve!r}, direction={direction!r})")
        self.knee = knee_convex_decreasing(x, y, S)
