"""CPU tier of the fused residual-block case matrix (tests/resblock_cases.py; the GPU tier is tests/test_gpu_resblocks.py).

(a) Source restatement.  The tiling constants and functions, the two support predicates, the launch grids
    (jg_resblock.hip, jg_resblock64.hip) and the conditions of ``resblock_second`` (jg_prepare.hip) that the negative cases
    meet are pinned as text; the Python restatement is evaluated against the pinned formulas.
(b) Coverage census.  From the ids and masks of every positive case alone: the output positions of each class
    (resblock_cases.CLASSES) - at least one for every class the case's shape can contain (resblock_cases.required_classes
    says which it cannot).
(c) Block reference and mutations.  The float64 block reference written the way the kernels tile it equals the two convs
    through oracle/ops.py; each mutation a wrong kernel could compute (shortcut from x m0; intermediate not multiplied by
    m1; not zero outside the row; a tile's outputs shifted by one; phase-split output not multiplied by m2) leaves the
    bounds of op_cases.check by 8x or more, in every case whose census counts its positions and at every geometry.
(d) Bounds.  The split-f16 emulation of the fused arithmetic stays 4x inside op_cases.GAMMA and RMS_BOUND at every geometry.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import conv_instance_cases as cc
import op_cases as oc
import resblock_cases as rc

CSRC = Path(__file__).resolve().parents[1] / "jaeger_amd" / "csrc"
EMU_MARGIN = 4.0
MUT_MARGIN = 8.0

_CENSUS, _MUT, _EMU = {}, {}, {}


def _norm(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return " ".join(text.replace("\\\n", " ").split())


@pytest.fixture(scope="module", autouse=True)
def tables():
    yield
    if _CENSUS:
        print("\ncoverage census (output positions per class; '.': the shape cannot contain it):")
        print("  " + f"{'case':36s}" + " ".join(f"{n[:9]:>9s}" for n in rc.CLASSES))
        for name, (counts, need) in _CENSUS.items():
            print("  " + f"{name:36s}" + " ".join(f"{counts[n] if (n in need or counts[n]) else '.':>9}" for n in rc.CLASSES))
    if _MUT:
        print("\nmutations (worst err / bound against the unmutated reference; >= %g required; '.': no such position):" % MUT_MARGIN)
        print("  " + f"{'case':36s}" + " ".join(f"{n:>12s}" for n in rc.MUTATIONS))
        for name, row in _MUT.items():
            print("  " + f"{name:36s}" + " ".join(f"{row[n]:12.3g}" if n in row else f"{'.':>12s}" for n in rc.MUTATIONS))
    if _EMU:
        print("\nmargins per geometry (emulation: worst err / bound <= %.3g, rms / RMS_BOUND <= %.3g; weakest mutation >= %g):"
              % (1 / EMU_MARGIN, 1 / EMU_MARGIN, MUT_MARGIN))
        for line in margins_table():
            print("  " + line)


def margins_table() -> list:
    out = []
    for g in rc.GEOMETRIES:
        names = [n for n in _EMU if rc.BY_NAME[n].geometry == g]
        if not names:
            continue
        worst = max(_EMU[n][0] for n in names)
        worst_m = max(_EMU[n][2] for n in names)
        rms = max(_EMU[n][1] for n in names) / oc.RMS_BOUND
        weakest = min((v, m, n) for n in names for m, v in _MUT.get(n, {}).items())
        out.append(f"c{g[0]} k{g[1]} d{g[2]:<2d} {len(names):2d} cases  emulation err/bound {worst:6.3f}  err/M {worst_m:8.2e} (GAMMA / {oc.GAMMA / worst_m:4.1f})"
                   f"  rms {rms:6.3f}   weakest mutation {weakest[0]:9.3g} ({weakest[1]})")
    return out


# ---- (a) the sources ---------------------------------------------------------------------------------------------------------
def test_tiling_and_predicates_match_the_sources():
    t32 = _norm((CSRC / "jg_resblock.hip").read_text())
    t64 = _norm((CSRC / "jg_resblock64.hip").read_text())
    const = lambda text, name: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))     # noqa: E731
    assert const(t32, "RB_NB") == rc.NB[32] and const(t64, "R6_NB") == rc.NB[64]
    assert const(t32, "RB_C") == 32 and const(t64, "R6_C") == 64
    assert const(t64, "R6_XR") == rc.XR and const(t64, "R6_OR") == rc.OR
    assert "constexpr int R6_RH = 32 * R6_NB;" in t64 and "constexpr int R6_PL = R6_CC * 4;" in t64 and "constexpr int R6_CC = R6_C / 16;" in t64
    assert ("void jg_resblock_tiling(int L, int k, int dil, int *nb, int *tile_out, int *tiles) { *nb = RB_NB; "
            "*tile_out = 32 * RB_NB - (k - 1) * dil; *tiles = (L + *tile_out - 1) / *tile_out; }") in t32
    assert ("void jg_resblock64_tiling(int L, int k, int dil, int *nb, int *tile_out, int *tiles) { *nb = R6_NB; "
            "*tile_out = R6_RH - (k - 1) * dil; *tiles = (L + *tile_out - 1) / *tile_out; }") in t64
    assert ("bool jg_resblock_supports(int c, int k, int dil) { return c == RB_C && (k == 5 || k == 3) && dil >= 1 && "
            "(k - 1) * dil <= 32; }") in t32
    assert ("bool jg_resblock64_supports(int c, int k, int dil) { return c == R6_C && (k == 5 || k == 3) && (dil == 1 || dil == 2) "
            "&& r6_smem(k, dil) <= 160 * 1024; }") in t64
    assert ("size_t r6_smem(int k, int dil) { const int RX = R6_RH + (k - 1) * dil; const int x_slot = (R6_PL * RX + 63) & ~63; "
            "return (size_t)(R6_XR * x_slot + 2 * R6_PL * R6_RH) * 16 + 4 * R6_C * sizeof(float) + (R6_OR * R6_RH + R6_OR) * "
            "sizeof(unsigned); }") in t64
    # the kernels' own geometry: halo, pad, the image rows
    assert "const int d = a.dil, halo = (RB_K - 1) * d, pad = halo / 2; constexpr int RH = 32 * RB_NB;" in t32
    assert "constexpr int d = RD, halo = (RK - 1) * d, pad = halo / 2; constexpr int RX = R6_RH + halo;" in t64
    # the grids
    assert "const long units = (long)a.rows * a.tiles_per_row; const int grid = (int)std::min<long>(units, 2L * e->n_cu);" in t32
    assert "const long units = (long)a.rows * a.tiles_per_row; const int grid = (int)std::min<long>(units, (long)e->n_cu);" in t64
    # the compiled instantiations: both tap counts at 32 channels, (5, 1) (5, 2) (3, 1) (3, 2) at 64
    assert set(re.findall(r"resblock32_kernel<(\d)>\)", t32)) == {"5", "3"}
    assert set(re.findall(r"launch\(resblock64_kernel<(\d), (\d)>\)", t64)) == {("5", "1"), ("5", "2"), ("3", "1"), ("3", "2")}
    # the restatement against the pinned formulas, over a grid of arguments
    for c in (16, 32, 64, 128):
        for k in (1, 3, 5, 7):
            for d in range(0, 20):
                assert rc.supports32(c, k, d) == (c == 32 and k in (3, 5) and d >= 1 and (k - 1) * d <= 32)
                rx = 64 + (k - 1) * d
                smem = (5 * ((16 * rx + 63) & ~63) + 2 * 16 * 64) * 16 + 4 * 64 * 4 + (3 * 64 + 3) * 4
                assert rc.supports64(c, k, d) == (c == 64 and k in (3, 5) and d in (1, 2) and smem <= 160 * 1024)
    for c, k, d in rc.GEOMETRIES:
        assert rc.supports(c, k, d)
        for l in (1, 57, 125, 300):
            t = rc.tiling(c, k, d, l)
            assert (t.nb, t.RH, t.halo, t.T, t.pad) == (rc.NB[c], 32 * rc.NB[c], (k - 1) * d, 32 * rc.NB[c] - (k - 1) * d, (k - 1) * d // 2)
            assert t.tiles == (l + t.T - 1) // t.T and t.halo == 2 * t.pad and t.T >= 1
    assert rc.grid(32, 1000, 256) == 512 and rc.grid(64, 1000, 256) == 256 and rc.grid(64, 100, 256) == 100
    # every d the 32-channel predicate accepts at its limit is in the matrix
    assert {(k, d) for c, k, d in rc.GEOMETRIES if c == 32} >= {(5, 1), (5, 8), (3, 1), (3, 16)}
    assert {(k, d) for c, k, d in rc.GEOMETRIES if c == 64} == {(5, 1), (5, 2), (3, 1), (3, 2)}


def test_negative_cases_meet_a_condition_of_resblock_second():
    text = _norm((CSRC / "jg_prepare.hip").read_text())
    body = text[text.index("static size_t resblock_second("):text.index("int jg_plan_resblocks(")]
    for c in rc.NEGATIVE:
        assert rc.NEG_RULES[c.neg] in body, (c.name, rc.NEG_RULES[c.neg])
    assert "if (!ok || ib == n || writer == ib) return n;" in body
    assert "hb.ep != (JG_EP_ADD | JG_EP_ACT1)" in body and "B.k != A.k || B.dilation != A.dilation" in body
    assert "B.out_buf == A.in_buf || B.out_buf == A.out_buf" in body
    by = {c.neg: c for c in rc.NEGATIVE}
    assert set(by) == set(rc.NEG_RULES) and len(rc.NEGATIVE) == len(rc.NEG_RULES)
    for reason in ("64 channels at dilation 3", "halo 36 > 32", "7 taps"):
        assert not rc.supports(*by[reason].geometry)
    for reason, c in by.items():                    # every other negative case has a geometry the kernels take
        if rc.NEG_RULES[reason] != rc._SUPPORTS:
            assert rc.supports(*c.geometry), c.name
    # the in-place case stays race-free layer by layer: one row-tiled tile a row
    c = by["conv2 writes in place"]
    assert c.l <= 256 and not cc.window_packed(k=c.k, dil=c.d, cout=c.c, stride=1, l=c.l, nw=c.n_win, ep=cc.ADD | cc.A1,
                                               strip_rows=False, as_k5=False, psplit=False, first=False)


def test_the_matrix_holds_what_it_promises():
    pos = rc.POSITIVE
    for g in rc.GEOMETRIES:
        T = rc.tiling(*g, 1).T
        mine = [c for c in pos if c.geometry == g and c.launch is None and c.chunk == 0 and c.store == "f16s" and c.masks != "none"]
        assert {c.l for c in mine} == {1, T, T + 1, 2 * T + 1}, g
        for l in (T + 1, 2 * T + 1):
            assert {c.masks for c in mine if c.l == l} == {"any", "strict"}, (g, l)
        assert {c.masks for c in mine} == {"any", "strict"}
    none = {c.geometry for c in pos if c.masks == "none"}
    assert {g for g in none if g[0] == 64} == {g for g in rc.GEOMETRIES if g[0] == 64}
    assert {g[1] for g in none if g[0] == 32} == {5, 3}
    for ch in (32, 64):
        ps = [c for c in pos if c.store == "psplit" and c.c == ch]
        assert len({c.geometry for c in ps}) == 2
        for g in {c.geometry for c in ps}:
            ls = [c.l for c in ps if c.geometry == g]
            assert sorted(l % 2 for l in ls) == [0, 1] and min(ls) > rc.tiling(*g, 1).T
    # launch shapes at the compute-unit counts of the devices in use: no multiple of the grid, the promised tiles a workgroup
    for n_cu in (256, 304, 64):
        for c in pos:
            if c.launch is None:
                assert 6 * c.n_win * c.til.tiles < rc.grid(c.c, 1 << 30, n_cu) or n_cu < 256
                continue
            nw = rc.launch_windows(c, n_cu)
            lo, hi = rc.n_local_range(c, nw, n_cu)
            assert hi == lo + 1 and c.til.tiles == 3, (c.name, lo, hi)
            if c.c == 32:
                assert lo >= 3
            want = {1.4: (1, 2), 2.4: (2, 3)}.get(c.launch)
            if want:
                assert (lo, hi) == want, (c.name, n_cu, lo, hi)
            if c.launch == 6.0:
                assert lo >= 6 and lo > rc.XR and lo > rc.OR
            # a few tens of MB: the F16S block tensors and the f32 readback
            assert nw * 6 * c.l * c.c * 4 < 40e6, (c.name, nw)
    assert {c.geometry for c in pos if c.launch == 6.0} == {g for g in rc.GEOMETRIES if g[0] == 64}
    assert sum(c.chunk == 2 and c.n_win == 5 for c in pos) == 2
    assert len(rc.GUARD) == 3 and {c.c for c in rc.GUARD} == {32, 64}


def test_tile_edge_ids_place_what_they_describe():
    """m0 (the 3-tap "any" mask of the ids) has runs of zeros beginning and ending at every position around T and 2 T."""
    from oracle import ops
    for c, k, d in rc.GEOMETRIES:
        t = rc.tiling(c, k, d, 1)
        l = 2 * t.T + 1
        ids = rc.tile_edge_ids(l, t.T, t.halo)
        assert ids.shape == (12, 6, l) and ids.dtype == np.uint8
        m0 = ops.mask_rule((ids != 0).astype(np.float64), 3, 1, 1, ops.PAD_SAME, ops.MASK_ANY).reshape(72, l)
        z = np.concatenate([np.ones((72, 1), bool), m0 != 0, np.ones((72, 1), bool)], axis=1)     # (valid outside the row)
        begins = (~z[:, 1:-1] & z[:, :-2]).any(axis=0)
        ends = (~z[:, 1:-1] & z[:, 2:]).any(axis=0)
        for B in (t.T, 2 * t.T):
            for q in range(B - t.halo - 1, min(B + t.halo + 1, l - 1) + 1):
                # (under the 3-tap "any" rule a masked position 1 / l - 2 has a masked row end beside it: no run begins / ends there)
                assert (begins[q] or q == 1) and (ends[q] or q == l - 2), (c, k, d, q)
        assert begins[0] and ends[l - 1]
        assert (ids[0] != 0).all() and (ids[1] == 0).all()
        cut = [(int(np.flatnonzero(ids[2, f] != 0).max()) + 1) for f in range(6)]
        assert all(1 <= q < t.T for q in cut) and all((ids[2, f, q:] == 0).all() for f, q in enumerate(cut))
        assert (ids != 0).mean() > 0.6                      # mostly valid codons all the same


# ---- (b) - (d) per case ------------------------------------------------------------------------------------------------------
def _worst(got, ref, M):
    return float((np.abs(got - ref) / (oc.GAMMA * M + oc.REL * np.abs(ref) + oc.FLOOR)).max())


@pytest.mark.parametrize("name", [c.name for c in rc.POSITIVE])
def test_case_census_mutations_and_emulation(name):
    from oracle import ops
    c = rc.BY_NAME[name]
    assert c.fused and rc.supports(*c.geometry)
    b = rc.build(c)
    prog = b.prog
    # every op evaluates, the outputs exist
    res = ops.run_program(prog, b.ids, keep=())
    assert set(res["vec"]) >= {ops.VEC_EMBEDDING, ops.VEC_PREDICTION}
    x, masks = rc.host_inputs(prog, b)
    assert x.shape == (c.n_win, 6, c.l, c.c)
    m0, m1, m2 = rc.block_masks(prog, b, masks, x.shape[:-1])
    assert float(np.abs(x[m0 == 0]).min() if (m0 == 0).any() else 1.0) > 1e-3      # x is non-zero where it is masked
    # (b) the census
    counts = rc.census(c, m0, m1, m2)
    need = rc.required_classes(c)
    _CENSUS[name] = (counts, need)
    assert not [n for n in need if counts[n] < 1], (name, {n: counts[n] for n in need})
    # (c) the block reference, tiled the kernels' way, is the two convs of oracle/ops.py
    ref, M = rc.chain_ref(prog, b, c, x, masks)
    mine = rc.block_ref(prog, b, c, x, masks)
    assert float(np.abs(mine - ref).max()) <= 1e-12 * max(1.0, float(np.abs(ref).max()))
    muts = rc.required_mutations(c, counts)
    row = {}
    for mut in muts:
        row[mut] = _worst(rc.block_ref(prog, b, c, x, masks, mutate=mut), ref, M)
    _MUT[name] = row
    weak = {m: v for m, v in row.items() if v < MUT_MARGIN}
    assert not weak, f"{name}: mutations that stay within {MUT_MARGIN}x the bound: {weak}"
    # (d) the fused arithmetic, emulated
    emu = rc.emulate_block(prog, b, c, x, masks)
    r = oc.check(emu, ref, M, f16s=True)
    _EMU[name] = (r.worst, r.rms, r.worst_m)
    assert r.worst * EMU_MARGIN <= 1.0 and r.rms * EMU_MARGIN <= oc.RMS_BOUND, r.report(f"{name} emulation")


def test_every_mutation_shows_at_every_geometry():
    """Runs behind the cases: a mutation without a case at some geometry means that geometry's ids are too weak."""
    if len(_MUT) < len(rc.POSITIVE):
        return
    for g in rc.GEOMETRIES:
        seen = {m for n, row in _MUT.items() if rc.BY_NAME[n].geometry == g for m in row}
        want = set(rc.MUTATIONS) - ({"no_m2"} if not any(c.store == "psplit" and c.geometry == g for c in rc.POSITIVE) else set())
        assert seen >= want, (g, want - seen)


@pytest.mark.parametrize("name", [c.name for c in rc.NEGATIVE + rc.GUARD])
def test_negative_and_guard_programs_evaluate(name):
    from oracle import ops
    c = rc.BY_NAME[name]
    b = rc.build(c)
    res = ops.run_program(b.prog, b.ids)
    assert set(res["vec"]) >= {ops.VEC_EMBEDDING, ops.VEC_PREDICTION}
    y = np.abs(res[b.conv2].out)
    h = np.abs(res[b.conv1].out)
    if c.guard:
        if c.gain1 > 100:           # only the intermediate leaves the f16 range: the block output stays far inside it
            assert float(h.max()) > 1e5 and float(y.max()) < 1e3, (float(h.max()), float(y.max()))
        else:
            assert float(y.max()) > 1e5 and float(h.max()) < 1e3, (float(h.max()), float(y.max()))
    else:
        assert float(y.max()) < 1e3 and np.isfinite(y).all()
