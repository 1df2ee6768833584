"""The fused whole-row kernels on the GPU against the float64 op interpreter chained from the ids (tests/fused_cases.py; bounds
and their margins: tests/test_fused_reference.py on the CPU): ``small_net_kernel`` through its pooled ``embedding`` and its NMD
taps, the table-net strand kernels (matrix-core and LDS-table form) through the pooled ``embedding``.  These kernels store no
tensor, so tests/test_gpu_op_taps.py cannot see them; tests/test_gpu_parity.py holds them to 1e-4 on pooled outputs of launch
groups in which no wave ever takes a second row.

Every case asserts the kernel it names ran (``placement()["small_fused"]`` / ``"table-net" in describe()``, one launch of its
profile class per forward) and every multi-row set that it took each wave (workgroup) round its row loop three times or more in
ONE launch.  Probe windows say where a fault sits: the offender list names the window = the start codon of its span.

The vector tail (part D): the pool, NMD-finish and first dense kernels of the layer-by-layer path are refused by the tap as
"outputs already"; here each is evaluated in float64 from the tensors the GPU itself produced (the tapped conv output and
mask, the GPU's own ``embedding`` / ``nmd``) and compared with the GPU's output vector.  Hidden vector slots (a head's inner
dense layers, NMD merge projections, the signals, the strand rows) are read through sibling models in tests/test_gpu_head.py.
"""
import time

import numpy as np
import pytest

import fused_cases as fc
import head_cases as hc
import op_cases as oc

pytestmark = pytest.mark.gpu

_TABLE = []
_T0 = time.time()


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    d.profile_enable(True)
    yield d
    print(f"\nfused-kernel margins (worst err/bound <= 1; rms err/M <= {fc.RMS_BOUND:.3g}, table net {fc.TAB_RMS_BOUND:.3g}):")
    for row in _TABLE:
        print("  " + row)
    print(f"  (module wall time {time.time() - _T0:.0f} s)")
    d.profile_enable(False)
    d.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _record(label, obs, res, rows):
    _TABLE.append(f"{label:46s} {obs:9s} rows {rows:6d}  worst {res.worst:8.3g}  rms err/M {res.rms:9.3g}  worst err/M {res.worst_m:9.3g}")


def _forward_one_group(device, model, ids, cls_name):
    """One forward as ONE launch group: returns the outputs; asserts exactly one launch of the profile class."""
    before = device.profile_read()[cls_name]["launches"]
    got = model.forward(ids, chunk=len(ids))
    after = device.profile_read()[cls_name]["launches"]
    assert after - before == 1, (cls_name, before, after)
    return got


# ---- small_net_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.SMALL_VARIANTS))
def test_small_net_kernel(device, n_cu, name):
    """Every variant (fused_cases.SMALL_VARIANTS says which compiled epilogue it is there for) on edge rows, probe windows at
    every codon, ragged windows and a multi-row set: embedding and every NMD tap within the bounds."""
    from jaeger_amd.engine import HipModel
    _, _, prog = fc.compile_small(name)
    net = fc.SmallNet(prog)
    model = HipModel(device, prog)
    failures = []
    try:
        model.set_precision("f16x3")
        assert model.placement()["small_fused"], model.describe()
        assert set(net.codes()) and (model.widths["nmd"] == 32 * len(net.finals))
        for set_name, ids in fc.small_input_sets(net, n_cu=n_cu).items():
            got = _forward_one_group(device, model, ids, "fused_small")
            rows = 6 * len(ids)
            sample = np.arange(len(ids))
            if set_name.startswith("multi-row"):
                grid = min(n_cu, (rows + 3) // 4)
                assert rows > 2 * 4 * grid and -(-rows // (4 * grid)) >= 4 and rows % (4 * grid) != 0, (rows, grid)
                _, cls = fc.multirow_ids(net.full_length(), n_cu)
                cov = fc.sequence_coverage(np.repeat(cls, 6), 4 * grid)
                assert cov["min_trips"] >= 3, cov
                assert min(cov[k] for k in ("full_short_full", "n_between", "probe_behind_full", "words_in_turn")) >= 1 or n_cu < 64, cov
                sample = fc.trip_sample(len(ids), 6, 4 * grid, cls)
                assert set(cls[sample]) == set(range(len(fc.ROW_CLASSES)))
            ref = fc.reference(prog, ids[sample])
            assert set(ref) == {"embedding"} | ({"nmd"} if net.finals else set())
            for obs, (r, mag) in ref.items():
                res, ok = fc.check_vec(got[obs][sample], r, mag)
                _record(f"{name} / {set_name}", obs, res, 6 * len(sample))
                if not ok:
                    res.offenders = [(int(sample[o[0]]),) + o[1:] for o in res.offenders]
                    failures.append(fc.report(f"{name} / {set_name} / {obs}", res))
        assert not failures, "\n".join(failures)
    finally:
        model.close()


def test_first_layer_second_affine_stays_off_the_fused_kernel(device):
    """conv0, BN, GELU, BN, GELU: the table layer's epilogue has no second affine, so such a model must run layer by layer (found
    by reading jg_small.hip beside prepare_small: the matcher took it and the kernel left the second BN + GELU out)."""
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    from oracle import forward as ofwd
    from oracle import ops
    cfg = fc.l0_aff2_cfg()
    prog = compile_plan(build_plan(cfg), ofwd.random_weights(cfg, seed=38341))
    assert fc.SmallNet(prog).layers[0]["aff2"]
    model = HipModel(device, prog)
    try:
        try:
            model.set_precision("f16x3")
        except L.JaegerHipError as exc:            # (off the fused kernel the model may have no split-f16 path at all:
            assert "split-f16 path unavailable" in str(exc), str(exc)      # any other refusal is not what this test is about)
            model.set_precision("f32")
        ids = oc.edge_ids(166, n_win=12)
        got = model.forward(ids)
        ref = ops.outputs(prog, ids)
        for k in ("embedding", "prediction"):
            assert float(np.abs(got[k] - ref[k]).max()) <= 1e-4, (k, float(np.abs(got[k] - ref[k]).max()))
        assert not model.placement()["small_fused"], model.describe()
    finally:
        model.close()


@pytest.mark.parametrize("name", ["nmdmerge500", "chain4"])
def test_small_rows_do_not_depend_on_their_wave_s_history(device, n_cu, name):
    """A multi-row set in one launch group and in groups of at most 64 windows (one trip per wave): bit-identical rows."""
    from jaeger_amd.engine import HipModel
    _, _, prog = fc.compile_small(name)
    net = fc.SmallNet(prog)
    model = HipModel(device, prog)
    try:
        model.set_precision("f16x3")
        assert model.placement()["small_fused"]
        ids, _ = fc.multirow_ids(net.full_length(), n_cu, seed=31)
        whole = _forward_one_group(device, model, ids, "fused_small")
        chunk = max(1, min(64, 4 * n_cu // 6))            # (a group this small: at most one trip per wave)
        before = device.profile_read()["fused_small"]["launches"]
        parts = model.forward(ids, chunk=chunk)
        assert device.profile_read()["fused_small"]["launches"] - before == -(-len(ids) // chunk)
        for k in whole:
            np.testing.assert_array_equal(whole[k], parts[k], err_msg=k)
    finally:
        model.close()


def test_small_predict_windows_equals_forward_on_a_multi_row_set(n_cu):
    """Both entry points launch the same kernel: ``predict_windows`` on bases = ``forward`` on the ids, bit for bit, on a set
    of full, short and N-holding windows that is one multi-row launch group."""
    from jaeger_amd.engine import JaegerHipEngine, frame_length
    from oracle import encoder as oenc
    cfg, weights, _ = fc.compile_small("nmdmerge500")
    rng = np.random.Generator(np.random.PCG64(37))
    fsize = 500
    n_win = int(np.ceil(3.4 * 4 * n_cu / 6)) + 1
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, fsize * n_win)].copy()
    seq[rng.random(seq.size) < 0.01] = ord("N")
    starts = (np.arange(n_win) * fsize).astype(np.int64)
    lens = np.full(n_win, fsize, np.int32)
    lens[1::3] = rng.integers(30, fsize, lens[1::3].size)
    for w in range(5, n_win, 11):
        seq[starts[w]:starts[w] + fsize] = ord("N")
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, precision="f16x3", chunk=n_win)
    try:
        assert eng.model.placement()["small_fused"]
        eng.device.profile_enable(True)
        got = eng.predict_windows(seq, starts, lens, fsize)
        assert eng.device.profile_read()["fused_small"]["launches"] == 1
        ids = oenc.encode_windows([seq[s:s + n].tobytes() for s, n in zip(starts, lens)], fsize, pad_to=frame_length(fsize))
        fwd = eng.model.forward(ids, chunk=n_win)
        assert 6 * n_win > 3 * 4 * n_cu
        for k in fwd:
            np.testing.assert_array_equal(got[k], fwd[k], err_msg=k)
    finally:
        eng.close()


# ---- the table-net strand kernels -------------------------------------------------------------------------------------------
def _strand_reference(prog, ids):
    """Per window: the mean of the two strand rows' pooled vectors (the ``embedding`` output of a two-strand model)."""
    ref, mag = fc.reference(prog, ids)["embedding"]
    return ref.reshape(len(ids), 2, -1).mean(axis=1), mag.reshape(len(ids), 2, -1).mean(axis=1)


@pytest.mark.parametrize("lds", [False, True], ids=["mfma", "lds"])
@pytest.mark.parametrize("name", list(fc.TAB_VARIANTS))
def test_table_net_kernels(device, n_cu, name, lds):
    """Max and average pool, every activation the kernels implement, VALID and SAME padding with dilation, both forms: rows of
    400, 131 and 37 bases, a multi-row set of rows of 200, and (matrix-core form asked for) rows of 1 200 bases, which only
    the LDS form fits."""
    from jaeger_amd.engine import HipModel
    _, _, prog = fc.compile_tab(name)
    model = HipModel(device, prog)
    failures = []
    try:
        device.set_table_net_lds(lds)
        assert "table-net" in model.describe(), model.describe()
        sets = {f"rows l={l}": fc.strand_ids(14, l) for l in (400, 131, 37)}
        sets["multi-row set l=200"] = fc.strand_multirow_ids(200, n_cu)
        if not lds and name == "dvf500":
            sets["rows l=1200"] = fc.strand_ids(8, 1200)
        for set_name, ids in sets.items():
            got = _forward_one_group(device, model, ids, "table")["embedding"]
            sample = np.arange(len(ids))
            if set_name.startswith("multi-row"):
                rows, grid = 2 * len(ids), (n_cu if lds else 2 * n_cu)
                assert rows >= 3 * grid + 1 and rows % grid != 0, (rows, grid)
                assert lds or (rows // grid) % 2 == 1          # (both parities of the id image end a workgroup's loop)
                sample = fc.trip_sample(len(ids), 2, grid)
            ref, mag = _strand_reference(prog, ids[sample])
            res, ok = fc.check_vec(got[sample], ref, mag, fc.TAB_GAMMA, fc.TAB_RMS_BOUND)
            _record(f"{name} {'lds' if lds else 'mfma'} / {set_name}", "embedding", res, 2 * len(sample))
            if not ok:
                res.offenders = [(int(sample[o[0]]),) + o[1:] for o in res.offenders]
                failures.append(fc.report(f"{name} / {set_name}", res, fc.TAB_GAMMA, fc.TAB_RMS_BOUND))
        assert not failures, "\n".join(failures)
    finally:
        device.set_table_net_lds(False)
        model.close()


def test_the_two_strand_forms_are_two_kernels(device):
    """Both forms run under the profile class "table", and the matrix-core form falls back to the LDS form without a sign (row
    too long, weights outside the f16 range).  On the average-pool variant the two differ in the order of the f32 sum and in the
    weights' hi / lo split: outputs that are bit-identical would mean the "mfma" cases above ran the LDS kernel twice."""
    from jaeger_amd.engine import HipModel
    _, _, prog = fc.compile_tab("avg_gelu")
    model = HipModel(device, prog)
    try:
        ids = fc.strand_ids(14, 400)
        device.set_table_net_lds(False)
        a = _forward_one_group(device, model, ids, "table")["embedding"]
        device.set_table_net_lds(True)
        b = _forward_one_group(device, model, ids, "table")["embedding"]
        assert not np.array_equal(a, b)
        assert float(np.abs(a - b).max()) <= 1e-5
    finally:
        device.set_table_net_lds(False)
        model.close()


@pytest.mark.parametrize("lds", [False, True], ids=["mfma", "lds"])
def test_strand_rows_do_not_depend_on_their_workgroup_s_history(device, n_cu, lds):
    """The strand kernels' multi-row set in one launch and in groups of 64 windows: bit-identical rows (the double-buffered id
    image of the matrix-core form, the id row and partial pools the LDS form reuses)."""
    from jaeger_amd.engine import HipModel
    _, _, prog = fc.compile_tab("dvf500")
    model = HipModel(device, prog)
    try:
        device.set_table_net_lds(lds)
        ids = fc.strand_multirow_ids(300, n_cu, seed=41)
        whole = _forward_one_group(device, model, ids, "table")
        parts = model.forward(ids, chunk=64)
        for k in whole:
            np.testing.assert_array_equal(whole[k], parts[k], err_msg=k)
    finally:
        device.set_table_net_lds(False)
        model.close()


# ---- part D: the vector tail from the GPU's own inputs ----------------------------------------------------------------------
# (the bounds - head_cases.gamma_sum / rms_sum, from the number formats - and the per-op loop live in tests/head_cases.py, which
# tests/test_gpu_head.py shares)
@pytest.mark.parametrize("name,precision,l", [("nmdmerge500", "f32", 100), ("nmdmerge500_max", "f32", 100),
                                              ("nmdmerge500", "f16x3", 300), ("nmdmerge500_max", "f16x3", 300),
                                              ("baseline500_nomask", "f32", 100), ("baseline500_nomaskmax", "f32", 100)])
def test_vector_tail_from_the_gpu_s_own_tensors(device, name, precision, l):
    """Layer by layer (exact f32 at any row length; split-f16 at rows too long for the fused kernel): the unfused POOL from the
    tapped output and mask of the last conv, every NMD finish from the tapped output of the conv whose last stage is the tap, and
    the dense layers that read ``embedding`` / ``nmd`` directly, each in float64 from what the GPU produced.  Average and max
    pool, the unmasked pool, an all-masked window (edge_ids window 10), the count + eps divide."""
    from jaeger_amd.engine import HipModel
    from test_gpu_op_taps import Taps
    _, _, prog = fc.compile_small(name)
    model = HipModel(device, prog)
    try:
        model.set_precision(precision)
        ids = oc.edge_ids(l, n_win=12)
        out = model.forward(ids)
        taps = Taps(model, ids, 0)
        checked = set()
        for i, what, res, ok in hc.tail_checks(prog, ids, out, taps, precision):
            checked.add(what)
            _record(f"tail {name} {precision} l={l} op {i} {what}", "", res, len(ids))
            assert ok, fc.report(f"{name} {precision} op {i} ({what})", res)
        # the pool is compared in every case but one: split-f16 fuses the max pool into a store-free conv (tests/test_gpu_op_taps.py)
        assert "dense" in checked and ("pool" in checked or (precision == "f16x3" and name.endswith("_max"))), checked
        if "nmdmerge" in name:
            assert "nmd finish" in checked
    finally:
        model.close()
