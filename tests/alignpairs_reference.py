"""TEST HELPER - CPU reference of ``jg_align_pairs``: a local alignment of two strings under the terminal-repeat scoring.

Score, columns, gaps in either row and the end cell are ``oracle.termini.smith_waterman``'s (it takes rectangular
inputs).  The identities, the aligned strings and the TIE FLAG come from this file's own traceback over its own
matrices: ``tied`` says that somewhere on the reported path two predecessors explained a cell (diagonal and a gap, two
gaps, or extending and opening a gap) - only then can another implementation with other preferences report another path.
"""

from __future__ import annotations

import numpy as np

from oracle import termini as ot

MATCH, MISMATCH, OPEN, EXT = ot.MATCH, ot.MISMATCH, ot.OPEN, ot.EXT
NEG = -10 ** 8
_COMPLEMENT = dict(zip("ATCG-NWSYRMKBVHD", "TAGC-NWSRYKMVBDH"))
_COMPLEMENT.update({"a": "T", "t": "A", "g": "C", "c": "G"})


def reverse_complement(seq: str) -> str:
    """The complement table of the reference's ``reverse_complement`` (lower-case acgt come back upper-case)."""
    return "".join(_COMPLEMENT.get(b, "N") for b in reversed(seq))


def _matrices(q: str, r: str):
    qa = np.frombuffer(q.upper().encode("latin-1"), np.uint8)
    ra = np.frombuffer(r.upper().encode("latin-1"), np.uint8)
    n, m = len(qa), len(ra)
    acgt = np.isin(ra, np.frombuffer(b"ACGT", np.uint8))
    H = np.zeros((n + 1, m + 1), np.int32)
    E = np.full((n + 1, m + 1), NEG, np.int32)
    F = np.full((n + 1, m + 1), NEG, np.int32)
    for i in range(1, n + 1):
        sub = np.where((ra == qa[i - 1]) & acgt, MATCH, MISMATCH)
        F[i, 1:] = np.maximum(F[i - 1, 1:] - EXT, H[i - 1, 1:] - OPEN)
        diag = H[i - 1, :-1] + sub
        e = NEG
        Hi, Ei, Fi = H[i], E[i], F[i]
        # E runs along the row: a plain loop, but only where a gap can be alive (a cell above the opening price behind it)
        hp = np.maximum(0, np.maximum(diag, Fi[1:]))
        if hp.max(initial=0) <= OPEN:
            Hi[1:] = hp
            continue
        h_left = 0
        for j in range(1, m + 1):
            e = max(e - EXT, h_left - OPEN)
            Ei[j] = e
            h_left = max(int(hp[j - 1]), e)
            Hi[j] = h_left
    return H, E, F


def align(query: str, ref: str, box_only: bool = False) -> dict:
    """-> score, cols, fgaps (gaps in the query row), rgaps, idents, end_q, end_r, query / ref / comp strings, tied.
    ``box_only``: this file's matrices are only filled over the cells between the alignment's first and last cell (whole
    flanks of 6 000 bases in a test that needs the strings, not the tie flag - which then only sees ties inside the box)."""
    sw = ot.smith_waterman(query, ref)
    out = {"score": sw["score"], "cols": sw["length"], "fgaps": sw["fgaps"], "rgaps": sw["rgaps"], "idents": 0,
           "end_q": sw["end_query"], "end_r": sw["end_ref"], "query": "", "ref": "", "comp": "", "tied": False}
    if sw["score"] == 0:
        return out
    if box_only:
        q0 = sw["end_query"] - (sw["length"] - sw["fgaps"]) + 1
        r0 = sw["end_ref"] - (sw["length"] - sw["rgaps"]) + 1
        query, ref = query[q0:sw["end_query"] + 1], ref[r0:sw["end_ref"] + 1]
        sw = dict(sw, end_query=len(query) - 1, end_ref=len(ref) - 1)
    H, E, F = _matrices(query, ref)
    assert int(H.max()) == sw["score"]
    i, j = sw["end_query"] + 1, sw["end_ref"] + 1
    assert int(H[i, j]) == sw["score"]
    qu, ru = query.upper(), ref.upper()
    a_q, a_r, comp, tied, state = [], [], [], False, "H"
    while True:
        if state == "H":
            if H[i, j] == 0:
                break
            same = qu[i - 1] == ru[j - 1] and qu[i - 1] in "ACGT"
            ways = [H[i, j] == H[i - 1, j - 1] + (MATCH if same else MISMATCH), H[i, j] == E[i, j], H[i, j] == F[i, j]]
            tied |= sum(bool(w) for w in ways) > 1
            if ways[0]:
                a_q.append(query[i - 1]); a_r.append(ref[j - 1]); comp.append("|" if same else " ")
                i, j = i - 1, j - 1
            else:
                state = "E" if ways[1] else "F"
        elif state == "E":
            a_q.append("-"); a_r.append(ref[j - 1]); comp.append(" ")
            ext, opn = E[i, j] == E[i, j - 1] - EXT, E[i, j] == H[i, j - 1] - OPEN
            tied |= bool(ext and opn)
            if not ext:
                state = "H"
            j -= 1
        else:
            a_q.append(query[i - 1]); a_r.append("-"); comp.append(" ")
            ext, opn = F[i, j] == F[i - 1, j] - EXT, F[i, j] == H[i - 1, j] - OPEN
            tied |= bool(ext and opn)
            if not ext:
                state = "H"
            i -= 1
    out.update(query="".join(reversed(a_q)), ref="".join(reversed(a_r)), comp="".join(reversed(comp)), tied=tied)
    out["idents"] = out["comp"].count("|")
    # the two tracebacks walk the same preferences: the counts agree
    assert (len(out["query"]), out["query"].count("-"), out["ref"].count("-")) == (out["cols"], out["fgaps"], out["rgaps"])
    return out


def result_row(a: dict) -> list[int]:
    """The eight numbers ``jg_align_pairs`` reports for this alignment."""
    return [a["score"], a["cols"], a["fgaps"], a["rgaps"], a["idents"], a["end_q"], a["end_r"], 0]


def align_jobs(bases, jobs) -> np.ndarray:
    """Stand-in for the device call: (n, 8) int32 for job records over a base buffer."""
    raw = bytes(np.asarray(bases, np.uint8))
    rows = np.zeros((len(jobs), 8), np.int32)
    for k, job in enumerate(jobs):
        q = raw[int(job["q_off"]):int(job["q_off"]) + int(job["q_len"])].decode("latin-1")
        r = raw[int(job["r_off"]):int(job["r_off"]) + int(job["r_len"])].decode("latin-1")
        if int(job["flags"]) & 1:
            r = reverse_complement(r)
        rows[k] = result_row(align(q, r, box_only=True))
    return rows
