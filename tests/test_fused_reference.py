"""The fused whole-row kernels' check on the CPU tier (tests/fused_cases.py; the GPU tier is tests/test_gpu_fused_kernels.py):

(a) oracle/ops.py gives a pool and an NMD finish a magnitude, and the variants between them reach every compiled epilogue of
    small_net_kernel (the switch of jg_small.hip) in both TAPS instantiations;
(b) numpy emulations of the kernels' arithmetic - small_net_kernel + small_pool_final_kernel, tab_mfma_kernel,
    tab_conv_pool_kernel - pass the check on every variant and input set, at least 4x inside the bounds;
(c) every mutation - the bugs such kernels typically have - fails it on at least one (input set, observable) pair by at least
    8x.  The errors, the margins and the pair that catches each mutation are printed (pytest -s).
"""
import numpy as np
import pytest

import fused_cases as fc
import op_cases as oc


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name):
        if name not in cache:
            _, _, prog = fc.compile_small(name)
            cache[name] = fc.SmallNet(prog)
        return cache[name]
    return get


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_pool_and_nmd_magnitudes():
    """OP_POOL / OP_NMD_FINAL carry M: the pool (mean, masked maximum) of the input's magnitude under the same mask, + |moving
    mean| for an NMD finish; |result| <= M everywhere, and an all-masked window has M = 0 under the max pool."""
    from oracle import ops
    for name in ("nmdmerge500", "nmdmerge500_max", "baseline500_nomask"):
        _, _, prog = fc.compile_small(name)
        ids = oc.edge_ids(166, n_win=12)
        keep = [i for i, op in enumerate(prog.ops) if op.kind in (ops.OP_POOL, ops.OP_NMD_FINAL)]
        res = ops.run_program(prog, ids, keep=keep)
        assert keep
        for i in keep:
            assert res[i].M is not None and res[i].M.shape == res[i].out.shape
            assert (np.abs(res[i].out) <= res[i].M * (1 + 1e-12) + 1e-300).all(), (name, i)
        pool = res[keep[-1]]
        if name != "baseline500_nomask":
            assert not pool.out[10].any() and not pool.M[10].any()          # the all-N window
            assert (pool.M[[0, 1, 2]] > 0).all()


def test_variants_reach_every_compiled_epilogue(nets):
    """The switch of small_net_kernel, the full product: codes 0 - 7 (second affine | add | save) and the four last-layer forms
    in both pool kinds, each with a tap (TAPS = true) and in a model without taps (TAPS = false: separately compiled and
    scheduled instances); the table layer with / without save and tap."""
    seen = set()
    for name in fc.SMALL_VARIANTS:
        net = nets(name)
        codes = net.codes()
        taps = any("t" in c for c in codes)
        seen |= {c if taps else "plain:" + c for c in codes}
        print(f"{name:20s} {' '.join(codes):28s} {fc.SMALL_VARIANTS[name]}")
    layer_codes = [str(c) for c in range(8)] + [f"{c}{m}" for c in (8, 10, 12, 14) for m in ("", "m")]
    want = {c.replace("m", "") + "t" + ("m" if c.endswith("m") else "") for c in layer_codes} | {"L0t", "L0st"}
    want |= {"plain:" + c for c in layer_codes + ["L0", "L0s"]}
    assert want <= seen, sorted(want - seen)
    assert max(nets(n).n_conv for n in fc.SMALL_VARIANTS) == 4 and min(nets(n).n_conv for n in fc.SMALL_VARIANTS) == 1
    assert max(len(nets(n).finals) for n in fc.SMALL_VARIANTS) == 5


def test_multirow_sets_hold_every_sequence():
    """A multi-row set takes every wave round its loop three times or more with an uneven tail, and the rows a wave meets in
    sequence hold every transition that exposes stale state - at a CU count of 256 as at 8."""
    for n_cu in (8, 64, 256, 304):
        ids, cls = fc.multirow_ids(166, n_cu)
        cov = fc.sequence_coverage(np.repeat(cls, 6), 4 * n_cu)
        assert ids.shape[0] * 6 > 2 * 4 * n_cu * 1.5 and cov["min_trips"] >= 3 and cov["max_trips"] == cov["min_trips"] + 1, cov
        assert set(cls) == set(range(len(fc.ROW_CLASSES)))
        for k in ("full_short_full", "n_between", "probe_behind_full", "words_in_turn"):
            assert cov[k] >= 1 or n_cu < 64, (n_cu, cov)     # (8 CUs - the CPU tier's own small set - hold 28 windows only)
    for n_cu in (256,):                                   # the strand kernels: one row per workgroup, 2 n_cu workgroups
        ids = fc.strand_multirow_ids(400, n_cu)
        assert ids.shape[0] * 2 >= 3 * 2 * n_cu + 1 and (ids.shape[0] * 2) % (2 * n_cu) != 0


# ---- (b), (c): the small-window kernel ------------------------------------------------------------------------------------
def _measure(net, ids, mut=None):
    ref = fc.reference(net.prog, ids)
    emu = fc.emulate_small(net, ids, mut)
    return {k: fc.check_vec(emu[k], r, m)[0] for k, (r, m) in ref.items()}


def test_emulation_passes_on_every_variant_and_input_set(nets):
    worst = dict(elem=(0.0, ""), rms=(0.0, ""), m=(0.0, ""))
    for name in fc.SMALL_VARIANTS:
        net = nets(name)
        for set_name, ids in fc.small_input_sets(net, n_cu=8, dense_probes=False).items():
            for obs, res in _measure(net, ids).items():
                what = f"{name} / {set_name} / {obs}"
                assert res.n_bad == 0 and res.rms <= fc.RMS_BOUND, fc.report(what, res)
                worst["elem"] = max(worst["elem"], (res.worst, what))
                worst["rms"] = max(worst["rms"], (res.rms, what))
                worst["m"] = max(worst["m"], (res.worst_m, what))
    print(f"emulation vs float64: worst err/bound {worst['elem'][0]:.3g} ({worst['elem'][1]}), worst err/M {worst['m'][0]:.3g} "
          f"({worst['m'][1]}), worst rms err/M {worst['rms'][0]:.3g} ({worst['rms'][1]}; RMS_BOUND {fc.RMS_BOUND:.3g})")
    assert worst["elem"][0] * 4 <= 1.0, worst["elem"]
    assert worst["rms"][0] * 4 <= fc.RMS_BOUND, worst["rms"]


#: the nets the mutations are tried on, in this order: taps on every layer first (each layer is seen through its own tap)
MUTATION_NETS = ("chain4", "mix_c", "nmdmerge500", "mix_d_max", "baseline500_max", "baseline500_nomask")


def _mutation_sets(net, mut):
    """Input sets for a mutation, cheapest first.  A mutation at one position: the probe windows whose span sees it."""
    l = net.full_length()
    short = 100
    if "pos" in mut:
        for ll in (l, short):
            l0 = net.geometry(ll)[0]
            if mut["pos"] < l0:
                starts = range(max(0, mut["pos"] - fc.SPAN - 8), min(ll, mut["pos"] + 9))
                yield f"probe windows (l = {ll})", fc.probe_ids(ll, starts=starts)
        yield f"edge rows (l = {l})", oc.edge_ids(l, n_win=12)
        return
    if mut["kind"] == "mask_carry":
        yield f"probe windows (l = {l})", fc.probe_ids(l, starts=range(40, 70))
    if mut["kind"] == "pool_beyond_l0":
        yield f"edge rows (l = {short})", oc.edge_ids(short, n_win=12)
        yield f"probe windows (l = {short})", fc.probe_ids(short, starts=range(short - 30, short))
    yield f"edge rows (l = {l})", oc.edge_ids(l, n_win=12)
    yield f"probe windows (l = {l})", fc.probe_ids(l, starts=range(0, l, 5))
    yield f"multi-row set (l = {l})", fc.multirow_ids(l, 8)[0]


def _strength(res):
    """How far beyond the bounds a result lies: err / element bound, RMS / RMS bound - whichever is larger."""
    return max(res.worst, res.rms / fc.RMS_BOUND)


def test_every_mutation_is_caught_by_8x(nets):
    caught = {}
    for name in MUTATION_NETS:
        net = nets(name)
        l0 = net.geometry(net.full_length())[0]
        for what, mut in fc.small_mutations(net, l0).items():
            if caught.get(what, (0,))[0] >= 8.0:
                continue
            best = caught.get(what, (0.0, ""))
            for set_name, ids in _mutation_sets(net, mut):
                for obs, res in _measure(net, ids, mut).items():
                    best = max(best, (_strength(res), f"{name} / {set_name} / {obs}: err/bound {res.worst:.3g}, err/M "
                                                      f"{res.worst_m:.3g}, rms err/M {res.rms:.3g}"))
                if best[0] >= 8.0:
                    break
            caught[what] = best
    weakest = min(caught.values())
    for what, (s, where) in sorted(caught.items(), key=lambda kv: kv[1][0]):
        print(f"{s:10.3g}x  {what}  <-  {where}")
    print(f"smallest mutation: {weakest[0]:.3g}x its bound (>= 8 required)")
    missed = [w for w, (s, _) in caught.items() if s < 8.0]
    assert not missed, missed
    assert len(caught) == 24 + 9          # (8 positions x 3 layers, and the nine faults of other kinds)


# ---- (b), (c): the table-net strand kernels ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tabs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fc.compile_tab(name)[2]
        return cache[name]
    return get


def _tab_measure(prog, ids, lds, mut=None):
    ref, mag = fc.reference(prog, ids)["embedding"]
    return fc.check_vec(fc.emulate_tab(prog, ids, lds, mut), ref, mag, fc.TAB_GAMMA, fc.TAB_RMS_BOUND)[0]


def test_table_net_emulations_pass(tabs):
    worst = dict(elem=(0.0, ""), rms=(0.0, ""))
    for name in fc.TAB_VARIANTS:
        for l in (400, 131, 37):
            ids = fc.strand_ids(14, l)
            for lds in (False, True):
                res = _tab_measure(tabs(name), ids, lds)
                what = f"{name} l={l} {'LDS' if lds else 'MFMA'}"
                assert res.n_bad == 0 and res.rms <= fc.TAB_RMS_BOUND, fc.report(what, res, fc.TAB_GAMMA, fc.TAB_RMS_BOUND)
                worst["elem"] = max(worst["elem"], (res.worst, what + f" (err/M {res.worst_m:.3g})"))
                worst["rms"] = max(worst["rms"], (res.rms, what))
    print(f"table-net emulations vs float64: worst err/bound {worst['elem'][0]:.3g} ({worst['elem'][1]}), worst rms err/M "
          f"{worst['rms'][0]:.3g} ({worst['rms'][1]}; TAB_RMS_BOUND {fc.TAB_RMS_BOUND:.3g})")
    assert worst["elem"][0] * 4 <= 1.0 and worst["rms"][0] * 4 <= fc.TAB_RMS_BOUND, worst


def test_table_net_mutations_are_caught_by_8x(tabs):
    for what, mut in fc.TAB_MUTATIONS.items():
        best = (0.0, "")
        for name in ("same_dil", "avg_gelu", "dvf500"):
            if mut == "same_as_valid_left" and name != "same_dil":
                continue
            for lds in (False, True):
                res = _tab_measure(tabs(name), fc.strand_ids(14, 131), lds, mut)
                s = max(res.worst, res.rms / fc.TAB_RMS_BOUND)
                best = max(best, (s, f"{name} l=131 {'LDS' if lds else 'MFMA'} / embedding: err/bound {res.worst:.3g}, rms err/M {res.rms:.3g}"))
        print(f"{best[0]:10.3g}x  {what}  <-  {best[1]}")
        assert best[0] >= 8.0, (what, best)
