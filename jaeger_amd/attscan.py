"""Att-site alignments on the GPU (``postprocess/prophages.py:800-814``: ``parasail.sw_trace_scan_16`` of the flank left of
a prophage region against the flank right of it, direct and reverse-complemented).

``jg_align_pairs`` (lengths up to 6 144) and ``jg_align_pairs_long`` (up to 12 288, every flank the report's rule can
produce) run every alignment of a call as one workgroup and return, per job, the score, the four counts of the
best path (columns, gaps in the query row, gaps in the reference row, identical columns) and its end cell - no traceback
matrix leaves the device.  The report also prints the aligned strings: :func:`traceback` rebuilds them on the host inside
the box the counts name (the alignment starts at ``end - consumed + 1`` in both sequences), with the kernel's recurrences
and tie rules, and refuses a box whose score or counts disagree with the kernel's.

Scoring (``parasail.matrix_create("ACGT", 2, -100)``, gap open 100 / extend 5): match +2, mismatch -100, a gap of k
columns costs 100 + 5 (k - 1); letters compare case-insensitively and only A/C/G/T can match.  Ties: H prefers the
diagonal, then the gap in the query row (E), then the gap in the reference row (F); E and F prefer extension; the best
cell is the first maximum in (column, row) order.  Which of several co-optimal alignments parasail reports is unpinned.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

MATCH, MISMATCH, OPEN, EXT = 2, -100, 100, 5
NEG = -10 ** 8
ALIGN_MAX = L.JG_ALIGN_MAX
ALIGN_LONG_MAX = L.JG_ALIGN_LONG_MAX
REVCOMP = L.JG_ALIGN_REVCOMP

#: one job of ``jg_align_pairs`` (32 bytes): spans of the base buffer, bit 0 of ``flags`` = reverse-complemented reference
JOB_DTYPE = np.dtype([("q_off", "<i8"), ("r_off", "<i8"), ("q_len", "<i4"), ("r_len", "<i4"), ("flags", "<i4"),
                      ("pad", "<i4")])
#: columns of a result row
SCORE, COLS, FGAPS, RGAPS, IDENTS, END_Q, END_R = range(7)

# seqops/transform.py:11-35: upper-case ambiguity codes complemented, lower-case a/c/g/t complemented to UPPER case,
# every other character N
_COMPLEMENT = dict(zip("ATCG-NWSYRMKBVHD", "TAGC-NWSRYKMVBDH"))
_COMPLEMENT.update({"a": "T", "t": "A", "g": "C", "c": "G"})


def reverse_complement(seq: str) -> str:
    return "".join(_COMPLEMENT.get(b, "N") for b in reversed(seq))


def make_jobs(rows) -> np.ndarray:
    """``rows``: (q_off, r_off, q_len, r_len, flags) tuples -> the job records."""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for k, (q_off, r_off, q_len, r_len, flags) in enumerate(rows):
        jobs[k] = (q_off, r_off, q_len, r_len, flags, 0)
    return jobs


def _device_call(entry: str, device, bases, jobs) -> np.ndarray:
    """One call of the C-ABI entry point ``entry`` (``jg_align_pairs`` or ``jg_align_pairs_long``: same arguments)."""
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    if not isinstance(bases, np.ndarray):
        bases = np.frombuffer(bases, np.uint8)
    bases = np.ascontiguousarray(bases, np.uint8)
    res = np.zeros((max(len(jobs), 1), 8), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L.check(getattr(device.lib, entry)(device.handle, ptr(bases), bases.size, L.JG_PTR_HOST, ptr(jobs), len(jobs), ptr(res)),
            entry)
    return res[:len(jobs)]


def align_pairs(device, bases, jobs) -> np.ndarray:
    """(n, 8) int32 from ``jg_align_pairs``: score, columns, query-row gaps, reference-row gaps, identities, end in the
    query, end in the reference, 0.  ``bases``: uint8 array or bytes; ``jobs``: :data:`JOB_DTYPE` records, each length
    1 .. :data:`ALIGN_MAX`."""
    return _device_call("jg_align_pairs", device, bases, jobs)


def align_pairs_long(device, bases, jobs) -> np.ndarray:
    """:func:`align_pairs` over ``jg_align_pairs_long``: each length 1 .. :data:`ALIGN_LONG_MAX`; a job whose two lengths are
    both at most :data:`ALIGN_MAX` gets the row :func:`align_pairs` returns."""
    return _device_call("jg_align_pairs_long", device, bases, jobs)


def align_flanks(device, bases, jobs) -> np.ndarray:
    """The report's device call, ONE call either way: all jobs through :func:`align_pairs` when no length exceeds
    :data:`ALIGN_MAX`, else all jobs through :func:`align_pairs_long`.  Both names are resolved in this module when the call
    is made (a test that replaces either still sees it); no job, no call."""
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    if len(jobs) == 0:
        return np.zeros((0, 8), np.int32)
    if max(int(jobs["q_len"].max()), int(jobs["r_len"].max())) > ALIGN_MAX:
        return align_pairs_long(device, bases, jobs)
    return align_pairs(device, bases, jobs)


def _codes(seq: str) -> np.ndarray:
    """A/C/G/T (any case) -> 0..3; everything else gets a code of its own position class that matches nothing."""
    raw = np.frombuffer(seq.encode("latin-1", "replace"), np.uint8)
    lut = np.full(256, 4, np.int8)
    for k, ch in enumerate("ACGT"):
        lut[ord(ch)] = lut[ord(ch.lower())] = k
    return lut[raw]


def box_matrices(query: str, ref: str):
    """H, E, F (int32, (n + 1, m + 1)) of the local alignment of ``query`` against ``ref``, row by row.  E needs no
    recursion along the row: a gap opened from a cell that was itself reached through that gap never beats extending
    it, so E[i][j] = max over k < j of (H'[i][k] - open - ext (j - 1 - k)), H' = max(0, diagonal, F) - a prefix maximum."""
    q, r = _codes(query), _codes(ref)
    n, m = len(q), len(r)
    H = np.zeros((n + 1, m + 1), np.int32)
    E = np.full((n + 1, m + 1), NEG, np.int32)
    F = np.full((n + 1, m + 1), NEG, np.int32)
    jj = np.arange(m + 1, dtype=np.int32)
    for i in range(1, n + 1):
        sub = np.where((r == q[i - 1]) & (r < 4), MATCH, MISMATCH).astype(np.int32)
        F[i, 1:] = np.maximum(F[i - 1, 1:] - EXT, H[i - 1, 1:] - OPEN)
        hp = np.zeros(m + 1, np.int32)
        hp[1:] = np.maximum(0, np.maximum(H[i - 1, :-1] + sub, F[i, 1:]))
        best_prev = np.maximum.accumulate(hp + EXT * jj)[:-1]
        E[i, 1:] = best_prev - OPEN - EXT * (jj[1:] - 1)
        H[i, 1:] = np.maximum(hp[1:], E[i, 1:])
    return H, E, F


def traceback(query: str, ref: str, row) -> dict:
    """Aligned strings of the alignment a result row of :func:`align_pairs` describes.  ``query`` / ``ref``: the two
    sequences of the job as the aligner saw them (``ref`` already reverse-complemented for such a job), in the file's own
    characters.  -> ``query``, ``ref`` (gaps ``-``), ``comp`` (``|`` at identical A/C/G/T columns, blank elsewhere),
    ``score``, ``end_query``, ``end_ref``.  Raises ``ValueError`` when the box disagrees with the row."""
    score, cols, fgaps, rgaps, idents, end_q, end_r = (int(v) for v in list(row)[:7])
    if score <= 0:
        return {"query": "", "ref": "", "comp": "", "score": 0, "end_query": -1, "end_ref": -1}
    q0, r0 = end_q - (cols - fgaps) + 1, end_r - (cols - rgaps) + 1      # a gap column consumes no base of its own row
    if q0 < 0 or r0 < 0 or end_q >= len(query) or end_r >= len(ref):
        raise ValueError(f"alignment box ({q0}..{end_q}, {r0}..{end_r}) outside the sequences")
    qs, rs = query[q0:end_q + 1], ref[r0:end_r + 1]
    qc, rc = _codes(qs), _codes(rs)
    H, E, F = box_matrices(qs, rs)
    i, j = len(qs), len(rs)
    if int(H[i, j]) != score or int(H.max()) != score:
        raise ValueError(f"alignment box scores {int(H[i, j])} at its end cell (maximum {int(H.max())}), the device {score}")
    out_q, out_r, out_c = [], [], []
    state = "H"
    while True:
        if state == "H":
            if H[i, j] == 0:
                break
            same = qc[i - 1] < 4 and qc[i - 1] == rc[j - 1]
            if H[i, j] == H[i - 1, j - 1] + (MATCH if same else MISMATCH):
                out_q.append(qs[i - 1]); out_r.append(rs[j - 1]); out_c.append("|" if same else " ")
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                state = "F"
        elif state == "E":                          # a reference base against a gap in the query row
            out_q.append("-"); out_r.append(rs[j - 1]); out_c.append(" ")
            if E[i, j] != E[i, j - 1] - EXT:
                state = "H"
            j -= 1
        else:                                       # a query base against a gap in the reference row
            out_q.append(qs[i - 1]); out_r.append("-"); out_c.append(" ")
            if F[i, j] != F[i - 1, j] - EXT:
                state = "H"
            i -= 1
    a_q, a_r, comp = "".join(reversed(out_q)), "".join(reversed(out_r)), "".join(reversed(out_c))
    got = (len(a_q), a_q.count("-"), a_r.count("-"), comp.count("|"))
    if (i, j) != (0, 0) or got != (cols, fgaps, rgaps, idents):
        raise ValueError(f"traceback gives (columns, query gaps, reference gaps, identities) = {got} from box cell "
                         f"({i}, {j}), the device {(cols, fgaps, rgaps, idents)}")
    return {"query": a_q, "ref": a_r, "comp": comp, "score": score, "end_query": end_q, "end_ref": end_r}
