"""The vector head's checks on the CPU tier (tests/head_cases.py; the GPU tier is tests/test_gpu_head.py):

(a) every sibling family compiles from ONE weight dict, the layer two siblings share has equal fields and equal weight bytes,
    and the restated launch rule of jg_launch_dense maps every case to the kernel it is there for;
(b) oracle/ops.py's run_op chained over every case computes oracle/forward.py's (oracle/strands.py's) network in float64;
(c) numpy float32 emulations of the kernels as their source states them pass the check at least 4x inside every bound, and
(d) every mutation - the bugs such kernels typically have - fails it on at least one case by at least 8x.  The margins and the
    case that catches each mutation are printed (pytest -s).
"""
import math

import numpy as np
import pytest
import torch

import fused_cases as fc
import head_cases as hc
import op_cases as oc

REL_CHAIN = 2e-9             # tests/test_op_reference.py's bound on the interpreter against the oracle's network


@pytest.fixture(scope="module")
def ids():
    return oc.edge_ids(hc.CODONS, n_win=hc.ROWS)


@pytest.fixture(scope="module")
def dense_cases(ids):
    """[(label, program, dense op, its f32 input rows)] of every layer of every family, with and without bias: the input is the
    float64 chain's value rounded to f32, as a sibling's output would hold it."""
    from oracle import ops
    cases = []
    for name in hc.DENSE_FAMILIES:
        for bias in (True, False):
            fam = hc.dense_family(name, bias)
            full = fam.progs[max(fam.progs)]
            res = ops.run_program(full, ids)
            x = res[next(i for i, o in enumerate(full.ops) if o.kind == ops.OP_POOL)].out.astype(np.float32)
            for i in hc.head_chain(full, ops.VEC_PREDICTION):
                op = full.ops[i]
                cases.append((f"{name}{'' if bias else ' no bias'} {op.cin}->{op.cout} {hc._act_name(op.arg) or 'linear'}", full, i, x))
                x = res[i].out.astype(np.float32)
    return cases


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_sibling_families_compile_from_one_weight_dict():
    """Heads [dense 500 gelu], [.., dense 77 tanh], [.., dense 257 sigmoid], [.., dense 3] from one dict: n_classes 500, 77, 257,
    3; the merge siblings: nmd_dim 10 beside 48 raw channels, an OODSIG at offset 10, a VECMAX of 2 x 10; the strand siblings."""
    from oracle import ops
    fam = hc.dense_family("w68_a")
    assert [fam.progs[j].n_classes for j in (1, 2, 3, 4)] == [500, 77, 257, 3]
    for name in hc.DENSE_FAMILIES:
        for bias in (True, False):
            fam = hc.dense_family(name, bias)
            for j, prog in fam.progs.items():
                assert len(hc.head_chain(prog, ops.VEC_PREDICTION)) == j
    for name, (taps, target, _) in hc.VECMAX_CASES.items():
        fam = hc.vecmax_family(name)
        d, v = hc.vecmax_ops(fam.progs["max"])
        raw = 24 * 2 + (40 if taps == 3 else 0)
        assert fam.progs["max"].nmd_dim == target and fam.progs["concat"].nmd_dim == raw
        assert (fam.progs["max"].ops[v].k, fam.progs["max"].ops[v].cout) == (taps, target)
        assert (fam.progs["max"].ops[d].cin, fam.progs["max"].ops[d].cout) == (raw, taps * target)
        assert not any(op.kind == ops.OP_VECMAX for op in fam.progs["concat"].ops)
    for name, (n_cls, nmd_dim, signals) in hc.OOD_CASES.items():
        fam, ids_, planted = hc.ood_family(name)
        prog = fam.progs["ood"]
        op = prog.ops[hc.ood_op(prog)]
        assert (op.cin, op.stride, op.vec_off, op.cout) == (n_cls, nmd_dim, nmd_dim, len(signals))
        assert prog.n_classes == n_cls and prog.nmd_dim == nmd_dim and len(ids_) == hc.ROWS + len(planted)
    assert {c[1] % 4 for c in hc.OOD_CASES.values()} == {0, 2}          # a signal offset that is no multiple of 4 among them
    sf = hc.strand_family()
    assert {k: p.n_classes for k, p in sf.progs.items()} == {"concat": 3, "average": 3, "sum": 3, "max": 3, "prefix": 500, "identity": 500}
    assert all(p.strands == 2 for p in sf.progs.values())


def test_shared_ops_have_equal_fields_and_weight_bytes():
    """Layer j of a prefix sibling (its last) is layer j of every longer sibling; the block-diagonal dense and the convs of a
    merge model are those of its concat sibling; the strand siblings share the branch and the head."""
    from oracle import ops
    for name in hc.DENSE_FAMILIES:
        fam = hc.dense_family(name)
        full = hc.head_chain(fam.progs[max(fam.progs)], ops.VEC_PREDICTION)
        for j, prog in fam.progs.items():
            mine = hc.head_chain(prog, ops.VEC_PREDICTION)
            for a, b in zip(mine, full):
                assert hc.op_fields(prog, a) == hc.op_fields(fam.progs[max(fam.progs)], b), (name, j)
    for fam in [hc.vecmax_family(n) for n in hc.VECMAX_CASES] + [hc.strand_family()]:
        progs = list(fam.progs.values())
        convs = [[(op.k, op.cin, op.cout, np.asarray(p.blob, np.float32)[op.w_off:op.w_off + 8].tobytes())
                  for op in p.ops if op.kind == ops.OP_CONV] for p in progs]
        assert all(c == convs[0] and c for c in convs)
    sf = hc.strand_family()
    chain = {k: hc.head_chain(p, ops.VEC_PREDICTION) for k, p in sf.progs.items()}
    for k in ("average", "sum", "max"):
        assert [hc.op_fields(sf.progs[k], i) for i in chain[k]] == [hc.op_fields(sf.progs["concat"], i) for i in chain["concat"]]
    assert hc.op_fields(sf.progs["prefix"], chain["prefix"][0]) == hc.op_fields(sf.progs["concat"], chain["concat"][0])
    eye = sf.progs["identity"].ops[chain["identity"][0]]
    assert eye.b_off < 0 and eye.arg == ops.ACT_NONE
    assert np.array_equal(np.asarray(sf.progs["identity"].blob, np.float32)[eye.w_off:eye.w_off + 250000].reshape(500, 500), np.eye(500))


def test_launch_rule_maps_each_case_to_its_kernel(dense_cases):
    """jg_launch_dense restated: every (cin -> cout) of ``head_cases.DENSE_WANT`` is a layer of some family and lands on the kernel it
    is there for in one launch group of 13 windows; under chunk 5 (groups of 5, 5, 3) no layer is tiled, narrow ones stay narrow;
    the LDS rule's edge sits between cin 1536 and 1540; every activation code a head layer can carry is there."""
    from oracle import ops
    seen, acts = {}, set()
    for _, prog, i, _ in dense_cases:
        op = prog.ops[i]
        seen[(op.cin, op.cout)] = hc.dense_kernel(hc.ROWS, op.cin, op.cout)
        acts.add(hc._act_name(op.arg))
        for nw in hc.groups_of(hc.ROWS, hc.CHUNK):
            k5 = hc.dense_kernel(nw, op.cin, op.cout)
            assert k5 != "tiled" and (k5 == "narrow") == (seen[(op.cin, op.cout)] == "narrow")
    for shape, want in hc.DENSE_WANT.items():
        assert seen.get(shape) == want, (shape, want, seen.get(shape))
    assert acts == hc.DENSE_ACTS
    assert hc.groups_of(hc.ROWS, hc.CHUNK) == [5, 5, 3] and hc.ROWS % hc.WT == 5
    assert hc.dense_kernel(8, 1536, 64) == "tiled" and hc.dense_kernel(8, 1537, 64) == "plain"
    assert hc.dense_kernel(7, 500, 500) == "plain" and hc.dense_kernel(10, 500, 500) == "tiled" and hc.dense_kernel(10, 500, 3) == "narrow"
    assert hc.dense_kernel(13, 63, 8) == "plain" and hc.dense_kernel(13, 64, 9) == "plain" and hc.dense_kernel(13, 64, 63) == "plain"
    # the restatement is pinned to the source: a changed launch rule must show here, not turn "plain against tiled" under
    # chunk 5 into tiled against tiled unnoticed
    from pathlib import Path
    src = " ".join((Path(__file__).resolve().parents[1] / "jaeger_amd" / "csrc" / "jg_kernels.hip").read_text().split())
    body = src[src.index("int jg_launch_dense("):src.index("// NMD finalisation")]
    for piece in ("constexpr int WT = 8;",
                  "if (cout >= 64 && cin >= 64 && n_win >= WT && (size_t)WT * ((cin + 3) & ~3) * sizeof(float) <= 48 * 1024) {",
                  "hipLaunchKernelGGL(dense_tiled_kernel<WT>,", "if (cout <= 8 && cin >= 64) {",
                  "hipLaunchKernelGGL(dense_narrow_kernel<8>,", "hipLaunchKernelGGL(dense_kernel,"):
        assert piece in body, piece
    assert body.index("dense_tiled_kernel<WT>") < body.index("dense_narrow_kernel<8>") < body.index("hipLaunchKernelGGL(dense_kernel,")
    sf = hc.strand_family()
    rows = [2 * w for w in hc.STRAND_WINDOWS]
    assert [hc.dense_kernel(r, 500, 500) for r in rows] == ["tiled", "plain"] and rows[0] % hc.WT == 2
    assert ops.OP_STRANDS == sf.progs["sum"].ops[-1].kind


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def _families():
    """(label, family, ids or None for the 13 edge windows of 40 codons) of EVERY case of head_cases."""
    for name in hc.DENSE_FAMILIES:
        for bias in (True, False):
            yield f"dense {name} bias {bias}", hc.dense_family(name, bias), None
    for name in hc.VECMAX_CASES:
        yield f"vecmax {name}", hc.vecmax_family(name), None
    for name in hc.OOD_CASES:
        fam, ids_, _ = hc.ood_family(name)
        yield f"ood {name}", fam, ids_
    for width in hc.POOL_WIDTHS:
        for pooling in ("max", "average"):
            for masked in (True, False):
                fam = hc.Family({"pool": hc.pool_cfg(width, pooling, masked)})
                for l in (hc.CODONS, 3):
                    yield f"pool {width} {pooling} {masked} l={l}", fam, oc.edge_ids(l, n_win=hc.ROWS)


def test_interpreter_computes_the_oracle_network_on_every_case(ids):
    from oracle import forward as ofwd
    from oracle import ops
    from oracle import strands as ost
    n = 0
    for label, fam, own_ids in _families():
        for key, prog in fam.progs.items():
            x = ids if own_ids is None else own_ids
            got = ops.outputs(prog, x)
            ref = ofwd.forward(fam.cfgs[key], fam.w, x, dtype=torch.float64)
            assert set(ref) <= set(got), (label, key, sorted(ref), sorted(got))
            for k, r in ref.items():
                r = np.asarray(r, np.float64)
                assert got[k].shape == r.shape, (label, key, k)
                assert float(np.abs(got[k] - r).max()) <= REL_CHAIN * max(1.0, float(np.abs(r).max())), (label, key, k)
                n += 1
    sf = hc.strand_family()
    sids = fc.strand_ids(5, hc.STRAND_BASES)
    for key, prog in sf.progs.items():
        got = ops.outputs(prog, sids)
        ref = ost.forward(sf.cfgs[key], sf.w, sids, dtype=torch.float64)
        for k, r in ref.items():
            assert r.dtype == np.float64 and got[k].shape == r.shape, (key, k)
            assert float(np.abs(got[k] - r).max()) <= REL_CHAIN * max(1.0, float(np.abs(r).max())), (key, k)
            n += 1
    assert n > 300


# ---- (c), (d) -------------------------------------------------------------------------------------------------------------
class Margins:
    """Per bound: the largest emulated err / bound and RMS / bound (headroom = 1 / it), the weakest mutation's distance."""

    def __init__(self):
        self.emu, self.mut, self.caught = {}, {}, {}

    def emulated(self, bound, label, res, rms_bound):
        assert res.n_bad == 0 and res.rms <= rms_bound, (bound, label, res.worst, res.rms, rms_bound)
        cur = self.emu.setdefault(bound, [0.0, "", 0.0, ""])
        if res.worst > cur[0]:
            cur[0], cur[1] = res.worst, label
        if res.rms / rms_bound > cur[2]:
            cur[2], cur[3] = res.rms / rms_bound, label

    def mutated(self, bound, mutation, label, res, rms_bound):
        d = hc.distance(res, rms_bound)
        if d > self.caught.get(mutation, (0.0, ""))[0]:
            self.caught[mutation] = (d, label, bound)
        self.mut[(bound, mutation)] = max(d, self.mut.get((bound, mutation), 0.0))

    def weakest(self, bound):
        """The nearest mutation among those this bound's cases see at all (distance > 1): none may sit between 1x and 8x."""
        seen = [(d, m) for (b, m), d in self.mut.items() if b == bound and d > 1.0]
        return min(seen) if seen else (math.inf, "-")

    def report(self):
        print("\nbound: emulation's headroom (element, RMS; >= 4x) | weakest mutation's distance (>= 8x)")
        for bound, (w, wl, r, rl) in self.emu.items():
            d, m = self.weakest(bound)
            print(f"  {bound:16s} {1 / max(w, 1e-300):9.3g}x ({wl})  {1 / max(r, 1e-300):9.3g}x ({rl}) | {d:9.3g}x ({m})")
        print("mutation: the case that catches it best")
        for mutation, (d, label, bound) in self.caught.items():
            print(f"  {mutation:66s} {d:9.3g}x  {label} [{bound}]")


def _bound_name(prog, i):
    return "dense " + (hc._act_name(prog.ops[i].arg) or "linear")


@pytest.fixture(scope="module")
def margins(ids, dense_cases):
    """Every emulation and every mutation against the float64 reference, once for the two tests below."""
    from oracle import ops
    mg = Margins()
    act_alone = mg.act_alone = {}
    # ---- dense: the three summation orders, one launch group and chunk 5
    for label, prog, i, x in dense_cases:
        op = prog.ops[i]
        for chunk in (0, hc.CHUNK):
            res, ok, gamma, rms = hc.check_dense(prog, i, x, hc.emulate_dense(prog, i, x, chunk))
            mg.emulated(_bound_name(prog, i), f"{label} chunk {chunk}", res, rms)
        name = hc._act_name(op.arg)
        if name in hc.ACT_GAMMA:                      # the activation alone: f32 against f64 on the same f32 sums
            pre = hc.emulate_dense(prog, i, x, preact=True)
            _, mag, _, _ = hc.dense_reference(prog, i, x)
            e = np.abs(hc.act32(op.arg, pre) - ops.act(op.arg, pre.astype(np.float64))) / np.maximum(mag, 2.0 ** -24)
            act_alone[name] = max(act_alone.get(name, 0.0), float(e.max()))
        assert np.array_equal(hc.emulate_dense(prog, i, x, 0), hc.emulate_dense(prog, i, x, hc.CHUNK)), \
            f"{label}: the emulated tiled and plain orders differ"
        for mut in hc.DENSE_MUTATIONS:
            res, ok, gamma, rms = hc.check_dense(prog, i, x, hc.emulate_dense(prog, i, x, 0, mut))
            mg.mutated(_bound_name(prog, i), mut, label, res, rms)
    # ---- vecmax
    for name in hc.VECMAX_CASES:
        fam = hc.vecmax_family(name)
        raw = ops.outputs(fam.progs["concat"], ids)["nmd"].astype(np.float32)
        prog = fam.progs["max"]
        ref, mag, gamma, rms = hc.vecmax_reference(prog, raw)
        bound = "vecmax " + (hc.VECMAX_CASES[name][2] or "linear")
        for chunk in (0, hc.CHUNK):
            res, _ = fc.check_vec(hc.emulate_vecmax(prog, raw, chunk), ref, mag, gamma, rms)
            mg.emulated(bound, name, res, rms)
        res, _ = fc.check_vec(hc.emulate_vecmax(prog, raw, 0, "vecmax striding groups by the padded width"), ref, mag, gamma, rms)
        mg.mutated(bound, "vecmax striding groups by the padded width", name, res, rms)
    # ---- the OOD signals
    for name, (n_cls, nmd_dim, signals) in hc.OOD_CASES.items():
        fam, oids, planted = hc.ood_family(name)
        prog = fam.progs["ood"]
        out = ops.outputs(prog, oids)
        logits, nmd = out["prediction"].astype(np.float32), out["nmd"].astype(np.float32)
        for q, (what, want) in enumerate(hc.planted_logits(n_cls).items()):     # the planted rows are the logits, bit for bit
            assert np.array_equal(logits[hc.ROWS + q], want.astype(np.float32)), (name, what)
        ref, mag = hc.ood_reference(prog, logits, nmd)
        assert np.isfinite(ref).all()
        emu = hc.emulate_oodsig(prog, logits, nmd)
        assert np.array_equal(emu[:, :nmd_dim], nmd)
        res, _ = fc.check_vec(emu[:, nmd_dim:], ref, mag, hc.SIG_GAMMA, hc.SIG_RMS)
        mg.emulated("signals", name, res, hc.SIG_RMS)
        for mut in hc.OOD_MUTATIONS:
            res, _ = fc.check_vec(hc.emulate_oodsig(prog, logits, nmd, mut)[:, nmd_dim:], ref, mag, hc.SIG_GAMMA, hc.SIG_RMS)
            mg.mutated("signals", mut, name, res, hc.SIG_RMS)
    # ---- pool and NMD finish: the conv output of the float64 chain rounded to f32, as the tap would return it
    for width in hc.POOL_WIDTHS:
        for pooling in ("average", "max"):
            for masked in (True, False):
                for l in (hc.CODONS, 3):
                    pids = oc.edge_ids(l, n_win=hc.ROWS)
                    prog = hc.Family({"pool": hc.pool_cfg(width, pooling, masked)}).progs["pool"]
                    taps = hc.OracleTaps(prog, pids)
                    pool = next(i for i, o in enumerate(prog.ops) if o.kind == ops.OP_POOL)
                    fin = next(i for i, o in enumerate(prog.ops) if o.kind == ops.OP_NMD_FINAL)
                    conv = next(i for i, o in enumerate(prog.ops) if o.kind == ops.OP_CONV)
                    x = taps.get(conv).reshape(len(pids), -1, width)
                    mk = taps.mask(pool, prog.ops[pool].in_mask)
                    assert (mk is not None) == masked
                    mm = np.asarray(prog.blob, np.float32)[prog.ops[fin].b_off:prog.ops[fin].b_off + width]
                    label = f"width {width} {pooling} {'masked' if masked else 'unmasked'} l={l}"
                    for mut in (None, "pool averaging over all positions instead of the mask count", "NMD finish dividing without eps"):
                        out = {"embedding": hc.emulate_pool(x, mk, pooling == "average", mut),
                               "nmd": hc.emulate_nmd_final(x, mk, mm, prog.ops[fin].f0, mut)}
                        out["prediction"], out["reliability"] = np.zeros((len(pids), 3), np.float32), np.zeros((len(pids), 1), np.float32)
                        for i, what, res, ok in hc.tail_checks(prog, pids, out, taps):
                            if what == "dense":
                                continue
                            n_pos = x.shape[1]
                            rms = hc.rms_sum(n_pos) if (what == "nmd finish" or pooling == "average") else 2.0 ** -24
                            bound = what + (" " + pooling if what == "pool" else "")
                            if mut is None:
                                mg.emulated(bound, label, res, rms)
                                if what == "pool" and pooling == "max":          # a maximum of given values: bit equality
                                    ref, _ = hc.pool_reference(prog, i, pids, taps)
                                    assert np.array_equal(out["embedding"], ref.out.astype(np.float32)), label
                            elif mut.startswith("pool") and what == "pool" and masked and pooling == "average":
                                mg.mutated(bound, mut, label, res, rms)
                            elif mut.startswith("NMD") and what == "nmd finish" and masked:
                                mg.mutated(bound, mut, label, res, rms)
    return mg


def test_bounds_sit_between_emulation_and_mutations(margins):
    """Per bound: the emulation sits >= 4x inside (element and RMS), the nearest mutation its cases see >= 8x beyond; the measured
    constants are powers of two >= 4x above the activation's (the signals') own emulated error."""
    mg = margins
    for name, worst in mg.act_alone.items():
        print(f"activation alone, {name}: largest err / M {worst:.3g}, ACT_GAMMA {hc.ACT_GAMMA[name]:.3g} = {hc.ACT_GAMMA[name] / worst:.3g}x")
        assert 4 * worst <= hc.ACT_GAMMA[name], (name, worst)
    assert set(mg.act_alone) == set(hc.ACT_GAMMA)
    mg.report()
    for c in list(hc.ACT_GAMMA.values()) + list(hc.ACT_RMS.values()) + [hc.SIG_GAMMA, hc.SIG_RMS]:
        assert math.log2(c).is_integer()
    want = {"dense " + (a or "linear") for a in hc.DENSE_ACTS} | {"signals", "nmd finish", "pool average", "pool max"}
    assert want <= set(mg.emu), want - set(mg.emu)
    for bound, (w, wl, r, rl) in mg.emu.items():
        assert 4 * w <= 1.0 and 4 * r <= 1.0, (bound, w, wl, r, rl)
        assert mg.weakest(bound)[0] >= 8.0, (bound, mg.weakest(bound))


def test_check_flags_every_mutation(margins):
    """Each mutation of the emulations fails the check on at least one case by >= 8x; the strand merge's by bit equality."""
    mg = margins
    print("\nmutation: the case that catches it best")
    for mutation, (d, label, bound) in mg.caught.items():
        print(f"  {mutation:66s} {d:9.3g}x  {label} [{bound}]")
    want = set(hc.DENSE_MUTATIONS) | set(hc.OOD_MUTATIONS) | {"vecmax striding groups by the padded width",
                                                               "pool averaging over all positions instead of the mask count",
                                                               "NMD finish dividing without eps"}
    assert set(mg.caught) == want, want ^ set(mg.caught)
    for mutation, (d, label, bound) in mg.caught.items():
        assert d >= 8.0, (mutation, d, label)
    # the strand merge on the module's own case: the concat sibling's per-strand logits and pooled vectors of the float64 chain,
    # rounded to f32 as the GPU's outputs hold them; the check is bit equality with head_cases.strand_expected
    from oracle import ops
    sf = hc.strand_family()
    sids = fc.strand_ids(hc.STRAND_WINDOWS[0], hc.STRAND_BASES)
    pred = ops.outputs(sf.progs["concat"], sids)["prediction"].astype(np.float32)
    emb = ops.outputs(sf.progs["identity"], sids)["prediction"].astype(np.float32)
    for a, b in ((pred[:, :3], pred[:, 3:]), (emb[:, :500], emb[:, 500:])):
        for kind in ("max", "sum", "average"):
            assert np.array_equal(hc.emulate_strand_merge(a, b, kind), hc.strand_expected(kind, a, b)), kind
        wrong = hc.emulate_strand_merge(a, b, "sum", "strand sum taken as max") != hc.strand_expected("sum", a, b)
        assert wrong.mean() > 0.9
        print(f"  {'strand sum taken as max':66s} bit equality: {int(wrong.sum())} of {wrong.size} elements differ "
              f"({a.shape[1]} columns of the concat / identity sibling)")
