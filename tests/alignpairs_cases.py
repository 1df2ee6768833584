"""TEST HELPER - the fixed case table of the rectangular local alignment (``jg_align_pairs`` / ``attscan.traceback``).

Every case is ``(name, query, ref, revcomp)``: with ``revcomp`` the aligner sees the reverse complement of ``ref``.
Hand-made cases (everything but ``fuzz_*``) are built so that their alignment is unique; the fuzz draws short repeats into
short random backgrounds, where a few co-optimal alignments are unavoidable (tests compare those on score and end cell).
"""

from __future__ import annotations

import numpy as np

from alignpairs_reference import reverse_complement

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def rand_seq(rng, n: int) -> str:
    return _ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _plant(rng, q_bg: int, r_bg: int, q_at: int, r_at: int, q_rep: str, r_rep: str, fence: str = "N"):
    """Random backgrounds with the repeats put in; ``fence`` on both sides of the query's copy (a letter that matches
    nothing) keeps the background from lengthening the repeat by chance."""
    q, r = rand_seq(rng, q_bg), rand_seq(rng, r_bg)
    return q[:q_at] + fence + q_rep + fence + q[q_at:], r[:r_at] + r_rep + r[r_at:]


def _mutate(rep: str, at: int) -> str:
    return rep[:at] + "ACGT"[("ACGT".index(rep[at]) + 1) % 4] + rep[at + 1:]


def hand_cases():
    rng = np.random.Generator(np.random.PCG64(20260))
    cases = []
    # planted exact repeats, 20 .. 600 long, rectangular backgrounds
    for L, qb, rb in ((20, 90, 140), (33, 200, 61), (64, 150, 150), (120, 300, 90), (251, 180, 320), (600, 260, 150)):
        rep = rand_seq(rng, L)
        q, r = _plant(rng, qb, rb, qb // 3, rb // 2, rep, rep)
        cases.append((f"exact_{L}", q, r, False))
    # one mismatch / one gap in either row, more than 50 matches on both sides
    rep = rand_seq(rng, 150)
    q, r = _plant(rng, 120, 200, 40, 77, rep, _mutate(rep, 70))
    cases.append(("mismatch", q, r, False))
    rep = rand_seq(rng, 160)
    q, r = _plant(rng, 140, 100, 30, 51, rep[:80] + rep[81:], rep)           # a base missing in the query: query-row gap
    cases.append(("query_gap", q, r, False))
    rep = rand_seq(rng, 170)
    q, r = _plant(rng, 100, 160, 60, 20, rep, rep[:90] + rep[93:])           # three bases missing in the reference
    cases.append(("ref_gap3", q, r, False))
    # lower case inside a repeat matches; N inside a repeat never does
    rep = rand_seq(rng, 90)
    q, r = _plant(rng, 100, 100, 10, 60, rep[:30] + rep[30:60].lower() + rep[60:], rep)
    cases.append(("lower_case", q, r, False))
    rep = rand_seq(rng, 180)
    q, r = _plant(rng, 80, 130, 33, 44, rep[:88] + "N" + rep[89:], rep[:88] + "N" + rep[89:])
    cases.append(("n_in_repeat", q, r, False))
    # reverse-complemented repeats: the reference span holds the repeat's reverse complement
    for L, qb, rb in ((40, 120, 200), (130, 210, 95)):
        rep = rand_seq(rng, L)
        q, r = _plant(rng, qb, rb, qb // 4, rb // 3, rep, reverse_complement(rep))
        cases.append((f"revcomp_{L}", q, r, True))
    rep = rand_seq(rng, 140)
    q, r = _plant(rng, 90, 90, 12, 70, rep, reverse_complement(rep[:64] + rep[65:]))
    cases.append(("revcomp_ref_gap", q, r, True))
    return cases


def fuzz_cases(n: int = 200):
    """Seeded fuzz of small pairs: a repeat of 14 .. 40 bases (sometimes with a mismatch or a missing base, sometimes
    reverse-complemented, sometimes none at all) in backgrounds of 1 .. 70 bases.  Repeats well above the background's
    chance matches keep the share of co-optimal alignments small."""
    rng = np.random.Generator(np.random.PCG64(4099))
    cases = []
    for k in range(n):
        qb, rb = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        kind = int(rng.integers(0, 6))
        rev = bool(rng.integers(0, 2))
        L = int(rng.integers(14, 41))
        rep = rand_seq(rng, L)
        q_rep = r_rep = rep
        if kind == 0:
            q_rep = r_rep = ""
        elif kind == 1:
            r_rep = _mutate(rep, int(rng.integers(0, L)))
        elif kind == 2:
            at = int(rng.integers(1, L - 1))
            r_rep = rep[:at] + rep[at + 1:]
        elif kind == 3:
            at = int(rng.integers(0, L))
            q_rep = rep[:at] + rep[at].lower() + rep[at + 1:]
        if rev:
            r_rep = reverse_complement(r_rep)
        q, r = _plant(rng, qb, rb, int(rng.integers(0, qb + 1)), int(rng.integers(0, rb + 1)), q_rep, r_rep, fence="")
        cases.append((f"fuzz_{k}", q, r, rev))
    return cases


def all_cases():
    return hand_cases() + fuzz_cases()
