"""Every kernel of the vector head on the GPU against oracle/ops.py's float64 evaluation of that op from the values the GPU itself
fed it (tests/head_cases.py: the sibling models, the cases, the bounds; tests/test_head_reference.py measures the bounds'
margins on the CPU): the three dense kernels at every shape of their launch rule and every activation code a head layer can
carry, the unfused POOL and NMD finish at widths whose 256 / (c / 4) is not whole or whose c exceeds 256, ``vecmax_kernel``,
``oodsig_kernel`` and ``strand_merge_kernel``.  A hidden vector slot is read as the exposed output of a sibling model compiled
from the same weight dict; the premise (``embedding`` / ``nmd`` bit-identical between siblings, equal fields and weight bytes of
the shared layer, the same kernel by the restated launch rule) is asserted in every test.

Rows of 40 codons (60 bases), 13 windows as ONE launch group - a full tile of 8 and a tail of 5 for ``dense_tiled_kernel<8>``,
a workgroup with three idle waves for ``dense_narrow_kernel<8>`` - and again in groups of 5, 5 and 3, where wide layers take the
plain kernel: bit-identical, as its comment promises.  Exact f32 throughout.

No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU call does not return.
"""
import faulthandler
import time

import numpy as np
import pytest

import fused_cases as fc
import head_cases as hc
import op_cases as oc

pytestmark = pytest.mark.gpu

_TABLE = []


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    t0 = time.time()                              # (from the first test's setup: the suite imports every module first)
    yield d
    print("\nvector head, per op (worst err/bound <= 1, rms err/M <= its bound):")
    for row in _TABLE:
        print("  " + row)
    print(f"  (module wall time {time.time() - t0:.1f} s)")
    d.close()


@pytest.fixture(scope="module")
def ids():
    return oc.edge_ids(hc.CODONS, n_win=hc.ROWS)


def _record(label, what, res, rms_bound=None):
    bound = "part D's" if rms_bound is None else f"{rms_bound:8.3g}"
    _TABLE.append(f"{label:52s} {what:18s} worst {res.worst:8.3g}  rms err/M {res.rms:9.3g} (bound {bound})  worst err/M {res.worst_m:9.3g}")


def _forwards(device, prog, ids, chunks):
    """One model, exact f32: its outputs per chunk size (0 = all windows as ONE launch group)."""
    from jaeger_amd.engine import HipModel
    model = HipModel(device, prog)
    try:
        model.set_precision("f32")
        return [model.forward(ids, chunk=c or len(ids)) for c in chunks]
    finally:
        model.close()


def _same(a: dict, b: dict, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


# ---- 1. dense -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", list(hc.DENSE_FAMILIES))
def test_dense_layers_from_their_sibling_exposed_inputs(device, ids, name, bias):
    """Layer j of a head: its input is the ``prediction`` of the sibling cut behind layer j - 1 (``embedding`` for the first),
    its output the ``prediction`` of the sibling cut behind layer j."""
    from oracle import ops
    fam = hc.dense_family(name, bias)
    n = max(fam.progs)
    full_chain = hc.head_chain(fam.progs[n], ops.VEC_PREDICTION)
    outs, outs5 = {}, {}
    for j, prog in fam.progs.items():
        outs[j], outs5[j] = _forwards(device, prog, ids, (0, hc.CHUNK))
    failures = []
    for j in range(1, n + 1):
        prog = fam.progs[j]
        i = hc.head_chain(prog, ops.VEC_PREDICTION)[-1]
        op = prog.ops[i]
        # the premise: same representation learner, same layer
        np.testing.assert_array_equal(outs[j]["embedding"], outs[n]["embedding"], err_msg=f"sibling {j}: embedding")
        assert hc.op_fields(prog, i) == hc.op_fields(fam.progs[n], full_chain[j - 1]), (name, j)
        assert (op.b_off >= 0) == bias and prog.n_classes == op.cout
        kernel = hc.dense_kernel(hc.ROWS, op.cin, op.cout)
        assert hc.DENSE_WANT.get((op.cin, op.cout), kernel) == kernel, (op.cin, op.cout, kernel)
        x = outs[j]["embedding"] if j == 1 else outs[j - 1]["prediction"]
        assert x.shape == (hc.ROWS, op.cin)
        res, ok, gamma, rms = hc.check_dense(prog, i, x, outs[j]["prediction"])
        _record(f"{name} {'bias' if bias else 'no bias'} {op.cin}->{op.cout} {hc._act_name(op.arg) or 'linear'}", kernel, res, rms)
        if not ok:
            failures.append(fc.report(f"{name} layer {j} ({op.cin}->{op.cout}, {kernel}; offenders: window, -, -, -, output)", res, gamma, rms))
        # groups of 5, 5 and 3: no tile of 8, so a wide layer runs on the plain kernel - the same sums in the same order
        assert all(hc.dense_kernel(nw, op.cin, op.cout) == ("narrow" if kernel == "narrow" else "plain")
                   for nw in hc.groups_of(hc.ROWS, hc.CHUNK))
        _same(outs5[j], outs[j], f"{name} sibling {j}, chunk {hc.CHUNK} against one launch group")
    assert not failures, "\n".join(failures)


# ---- 2. POOL and NMD finish, unfused -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("pooling", ["average", "max"])
@pytest.mark.parametrize("width", hc.POOL_WIDTHS)
def test_pool_and_nmd_finish_at_odd_widths(device, width, pooling, masked):
    """tests/test_gpu_fused_kernels.py part D, generalised: the pool from the tapped conv output and mask, the NMD finish from the
    tapped output of the conv whose last stage is its tap, the two dense layers from ``embedding`` / ``nmd``; rows of 40 codons
    and of 3 (fewer positions than position groups); window 10 is all N.  The max pool is also held to bit equality."""
    from jaeger_amd.engine import HipModel
    from oracle import ops
    from test_gpu_op_taps import Taps
    prog = hc.Family({"pool": hc.pool_cfg(width, pooling, masked)}).progs["pool"]
    assert 256 % (width // 4) != 0 or width > 256
    model = HipModel(device, prog)
    try:
        model.set_precision("f32")
        for l in (hc.CODONS, 3):
            pids = oc.edge_ids(l, n_win=hc.ROWS)
            out = model.forward(pids, chunk=len(pids))
            taps = Taps(model, pids, len(pids))
            checked = set()
            for i, what, res, ok in hc.tail_checks(prog, pids, out, taps):
                checked.add(what)
                _record(f"width {width} {pooling} {'masked' if masked else 'unmasked'} l={l} op {i}", what, res)
                assert ok, fc.report(f"width {width} {pooling} masked {masked} l={l} op {i} ({what})", res)
            assert checked == {"pool", "nmd finish", "dense"}, checked
            if pooling == "max":                           # a maximum of the tapped f32 values is one of them: no bound, bit equality
                i = next(i for i, op in enumerate(prog.ops) if op.kind == ops.OP_POOL)
                ref, _ = hc.pool_reference(prog, i, pids, taps)
                np.testing.assert_array_equal(out["embedding"], ref.out.astype(np.float32), err_msg=f"max pool, width {width}, l={l}")
            if masked:
                assert not out["embedding"][10].any()          # the all-N window pools to zeros
    finally:
        model.close()


# ---- 3. VECMAX ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hc.VECMAX_CASES))
def test_vecmax_from_the_concat_sibling(device, ids, name):
    """NMDMerge(max): the block-diagonal dense in float64 from the concat sibling's ``nmd``, then the maximum over the groups."""
    fam = hc.vecmax_family(name)
    got, got5 = _forwards(device, fam.progs["max"], ids, (0, hc.CHUNK))
    raw, raw5 = _forwards(device, fam.progs["concat"], ids, (0, hc.CHUNK))
    for k in ("embedding", "prediction"):                     # the premise: the same representation learner
        np.testing.assert_array_equal(got[k], raw[k], err_msg=k)
    prog = fam.progs["max"]
    d, v = hc.vecmax_ops(prog)
    assert raw["nmd"].shape == (hc.ROWS, prog.ops[d].cin) and got["nmd"].shape == (hc.ROWS, prog.ops[v].cout)
    ref, mag, gamma, rms = hc.vecmax_reference(prog, raw["nmd"])
    res, ok = fc.check_vec(got["nmd"], ref, mag, gamma, rms)
    _record(f"vecmax {name}", "dense " + hc.dense_kernel(hc.ROWS, prog.ops[d].cin, prog.ops[d].cout) + " + max", res, rms)
    assert ok, fc.report(f"vecmax {name}", res, gamma, rms)
    _same(got5, got, f"{name}, chunk {hc.CHUNK}")
    _same(raw5, raw, f"{name} concat, chunk {hc.CHUNK}")


# ---- 4. OODSIG ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hc.OOD_CASES))
def test_ood_signals_from_the_gpu_s_own_logits_and_nmd(device, name):
    """An identity reliability head shows [nmd | signals]; the reference is oracle/ops.py's ``_signals`` on the GPU's own
    ``prediction`` and ``nmd``: 13 random windows and the planted ones (equal maxima, the maximum first and last, the eps clamp,
    logits near +-80 and at the ends of exp's f32 range)."""
    n_cls, nmd_dim, signals = hc.OOD_CASES[name]
    fam, oids, planted = hc.ood_family(name)
    prog = fam.progs["ood"]
    out, out5 = _forwards(device, prog, oids, (0, hc.CHUNK))
    rel = out["reliability"]
    assert rel.shape == (len(oids), nmd_dim + len(signals)) and out["nmd"].shape == (len(oids), nmd_dim)
    np.testing.assert_array_equal(rel[:, :nmd_dim], out["nmd"])               # the premise: the identity head copies
    for q, (what, want) in enumerate(hc.planted_logits(n_cls).items()):
        np.testing.assert_array_equal(out["prediction"][hc.ROWS + q], want.astype(np.float32), err_msg=what)
    ref, mag = hc.ood_reference(prog, out["prediction"], out["nmd"])
    res, ok = fc.check_vec(rel[:, nmd_dim:], ref, mag, hc.SIG_GAMMA, hc.SIG_RMS)
    _record(f"ood {name}", "oodsig", res, hc.SIG_RMS)
    assert ok, fc.report(f"ood {name} (offenders: window, -, -, -, signal; planted windows from {hc.ROWS}: {planted})", res,
                         hc.SIG_GAMMA, hc.SIG_RMS)
    _same(out5, out, f"{name}, chunk {hc.CHUNK}")


# ---- 5. strand merge ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strand_family():
    return hc.strand_family()


@pytest.mark.parametrize("n_win", hc.STRAND_WINDOWS)
def test_strand_merge_and_the_500_to_500_layer(device, strand_family, n_win):
    """The dvf500 layout at 60 bases.  With two strands the f32 merge is unique: max = np.maximum(a, b), sum = a + b, average =
    (a + b) / 2 in numpy float32, bit for bit, from the concat sibling's per-strand vectors; ``embedding`` = the average of the
    identity sibling's.  The 500 -> 500 layer per strand row in float64 from the identity sibling's rows (10 rows: tiled with a
    tail of 2; 6 rows: the plain kernel), the 500 -> 3 layer from the prefix sibling's."""
    from oracle import ops
    fam = strand_family
    sids = fc.strand_ids(n_win, hc.STRAND_BASES)
    outs = {k: _forwards(device, p, sids, (0,))[0] for k, p in fam.progs.items()}
    for k in outs:                                              # the premise: one branch, one pooled vector
        np.testing.assert_array_equal(outs[k]["embedding"], outs["concat"]["embedding"], err_msg=k)
    a, b = outs["concat"]["prediction"][:, :3], outs["concat"]["prediction"][:, 3:]
    assert outs["concat"]["prediction"].shape == (n_win, 6)
    for kind in ("max", "sum", "average"):                      # np.maximum(a, b), a + b, (a + b) / 2 in numpy float32
        np.testing.assert_array_equal(outs[kind]["prediction"], hc.strand_expected(kind, a, b), err_msg=kind)
    ea, eb = outs["identity"]["prediction"][:, :500], outs["identity"]["prediction"][:, 500:]
    assert outs["identity"]["prediction"].shape == (n_win, 1000)
    np.testing.assert_array_equal(outs["concat"]["embedding"], hc.strand_expected("average", ea, eb))
    rows = 2 * n_win
    want = "tiled" if rows >= hc.WT else "plain"
    assert hc.dense_kernel(rows, 500, 500) == want and (rows % hc.WT == 2 or want == "plain")
    chain = {k: hc.head_chain(p, ops.VEC_PREDICTION) for k, p in fam.progs.items()}
    assert hc.op_fields(fam.progs["prefix"], chain["prefix"][0]) == hc.op_fields(fam.progs["concat"], chain["concat"][0])
    x = outs["identity"]["prediction"].reshape(rows, 500)
    h = outs["prefix"]["prediction"].reshape(rows, 500)
    y = outs["concat"]["prediction"].reshape(rows, 3)
    for label, prog, i, src, got in (("500->500 relu", fam.progs["prefix"], chain["prefix"][0], x, h),
                                      ("500->3 linear", fam.progs["concat"], chain["concat"][1], h, y)):
        op = prog.ops[i]
        res, ok, gamma, rms = hc.check_dense(prog, i, src, got)
        _record(f"strands {n_win} windows {label}", hc.dense_kernel(rows, op.cin, op.cout), res, rms)
        assert ok, fc.report(f"strands {n_win} windows {label} (offenders: strand row, -, -, -, output)", res, gamma, rms)
