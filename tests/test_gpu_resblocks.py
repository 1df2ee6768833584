"""The fused residual-block kernels on the GPU, case by case (tests/resblock_cases.py; its CPU tier,
tests/test_resblock_reference.py, pins the restated tiling to the sources, counts what every case's ids and masks cover and
shows that every mutation of the block leaves the bounds).  Per positive case, on a model in f16x3 with the fusion on:

* placement: ``describe()`` puts conv2 on the fused block, conv1's tap is refused with the message that names
  JG_OPT_FUSE_RESBLOCK 0, conv2's tap variant carries TAP_FUSED_RESBLOCK | TAP_F16S and TAP_PHASE_SPLIT exactly for a
  phase-split store;
* value: the tapped block output against both convs in float64 from the tapped block input and masks, with op_cases.check
  and its constants unchanged (a phase-split store times its output mask); the stride-2 readers of a phase-split store from
  the tapped block output;
* against the layer-by-layer path: with the fusion off the same program is checked conv by conv, and the two block outputs
  agree within the sum of their two bounds;
* bit for bit: a chunked forward equals the unchunked one; in the launch-shape cases a window duplicated at the end of the
  launch gives the rows of its first copy - a tile's result does not depend on the workgroup, pipeline step or ring slot.

Negative cases are not fused, conv1 can be tapped and every conv passes its per-op check.  The range-guard cases fall back to
exact f32 and then equal a model created in f32 bit for bit.
"""
import time

import numpy as np
import pytest

import op_cases as oc
import resblock_cases as rc
from test_gpu_op_taps import Taps

pytestmark = pytest.mark.gpu

_TABLE = []
_T0 = [None]


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    d.set_fuse_resblock(True)
    _T0[0] = time.time()
    yield d
    d.set_fuse_resblock(True)
    print("\nfused residual-block margins (worst err/bound <= 1; rms err/M <= %.3g):" % oc.RMS_BOUND)
    for row in _TABLE:
        print("  " + row)
    print("  (module wall time %.0f s)" % (time.time() - _T0[0]))
    d.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _record(label, res):
    _TABLE.append(f"{label:52s} worst {res.worst:8.3g}  rms err/M {res.rms:9.3g}  worst err/M {res.worst_m:9.3g}")


def _guarded(name, fn):
    """A HIP call that failed (a fault, a lost device) ends the session: nothing more runs on the device.  A refusal of the
    library itself is a finding and fails this test alone."""
    from jaeger_amd import _lib as L
    try:
        fn()
    except L.JaegerHipError as exc:
        if f"failed ({L.JG_ERR_HIP})" in str(exc):
            pytest.exit(f"{name}: {exc}", returncode=3)
        raise


def _conv_line(model, i):
    lines = [ln for ln in model.describe().splitlines() if ln.startswith(f"op {i}: conv")]
    assert len(lines) == 1, model.describe()
    return lines[0]


def _check_op(taps, i, label, failures):
    """Conv op i against oracle/ops.run_op from its producers' taps; returns (tapped tensor, reference, bound per element)."""
    from jaeger_amd import _lib as L
    from oracle import ops
    prog = taps.prog
    st = taps.state(i)
    got = taps.get(i)
    ref = ops.run_op(prog, i, st)
    out, M = ref.out, ref.M
    if taps.variant[i] & L.TAP_PHASE_SPLIT:
        om = st.mask[prog.ops[i].out_mask][..., None]
        out, M = out * om, M * om
    res = oc.check(got, out, M, f16s=bool(taps.variant[i] & L.TAP_F16S))
    _record(label, res)
    if not res.ok:
        failures.append(res.report(label))
    return got, out, oc.GAMMA * M + oc.REL * np.abs(out) + oc.FLOOR


def _block_inputs(taps, b):
    x = taps.get(b.feeder)
    masks = {taps.prog.ops[i].out_mask: taps.get(i) for i in b.masks}
    return x, masks


def _positive(device, c, n_win):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    b = rc.build(c, n_win)
    ids = b.ids
    dup = []
    if c.launch is not None:               # two windows again at the end of the launch: other workgroups, steps and ring slots
        dup = [(len(ids) - 1, 0), (len(ids) - 2, 4)]
        for dst, src in dup:
            ids[dst] = ids[src]
    prog = b.prog
    device.set_fuse_resblock(True)
    model = HipModel(device, prog)
    failures = []
    try:
        assert model.precision == "f16x3", model.describe()
        if not c.fused:                    # an earlier placement rule keeps the geometry off the kernel: not fused, right layer by layer
            assert "fused residual block" not in model.describe() and _placed_rule(c) in model.describe()
            taps = Taps(model, ids, c.chunk)
            for i in (b.conv1, b.conv2):
                _check_op(taps, i, f"{c.name} op {i} (not fused)", failures)
            assert not failures, "\n".join(failures)
            return
        # placement
        assert "fused residual block" in _conv_line(model, b.conv2), model.describe()
        assert ("phase-split store" in _conv_line(model, b.conv2)) == (c.store == "psplit"), model.describe()
        assert "computed by the block's second conv" in _conv_line(model, b.conv1), model.describe()
        with pytest.raises(L.JaegerHipError, match="fused residual block") as exc:
            model.tap(b.conv1, ids, chunk=c.chunk)
        assert "JG_OPT_FUSE_RESBLOCK 0" in str(exc.value), str(exc.value)
        taps = Taps(model, ids, c.chunk)
        y = taps.get(b.conv2)
        want = L.TAP_FUSED_RESBLOCK | L.TAP_F16S | (L.TAP_PHASE_SPLIT if c.store == "psplit" else 0)
        got_bits = taps.variant[b.conv2] & (L.TAP_FUSED_RESBLOCK | L.TAP_F16S | L.TAP_PHASE_SPLIT | L.TAP_EXACT_F32)
        assert got_bits == want, (c.name, hex(taps.variant[b.conv2]))
        # value: both convs in float64 from the tapped block input and masks
        x, masks = _block_inputs(taps, b)
        ref, M = rc.chain_ref(prog, b, c, x, masks)
        res = oc.check(y, ref, M, f16s=True)
        _record(f"{c.name} ({len(ids)} windows)", res)
        if not res.ok:
            failures.append(res.report(c.name))
        bound_f = oc.GAMMA * M + oc.REL * np.abs(ref) + oc.FLOOR
        for r in b.readers:
            _check_op(taps, r, f"{c.name} reader op {r}", failures)
        # bit for bit
        if c.chunk:
            np.testing.assert_array_equal(model.tap(b.conv2, ids, chunk=0), y, err_msg=f"{c.name}: chunk {c.chunk} against chunk 0")
        for dst, src in dup:
            np.testing.assert_array_equal(y[dst], y[src], err_msg=f"{c.name}: window {src} again as window {dst}")
        # the layer-by-layer path on the same model
        device.set_fuse_resblock(False)
        plain = Taps(model, ids, c.chunk)
        for i in [b.feeder] + b.masks:       # (the ops in front of the block do not depend on the option)
            plain.cache[i], plain.variant[i] = taps.cache[i], taps.variant[i]
        _check_op(plain, b.conv1, f"{c.name} conv1 layer by layer", failures)
        y2, _, bound_u = _check_op(plain, b.conv2, f"{c.name} conv2 layer by layer", failures)
        assert not plain.variant[b.conv2] & L.TAP_FUSED_RESBLOCK and not plain.variant[b.conv1] & L.TAP_FUSED_RESBLOCK
        gap = np.abs(y.astype(np.float64) - y2) / (bound_f + bound_u)
        if float(gap.max()) > 1.0:
            idx = np.unravel_index(int(gap.argmax()), gap.shape)
            failures.append(f"{c.name}: fused and layer-by-layer outputs differ by {float(gap.max()):.3g} x the sum of their bounds at "
                            f"(row, frame, position, channel) {tuple(int(v) for v in idx)}")
        assert not failures, "\n".join(failures)
    finally:
        device.set_fuse_resblock(True)
        model.close()


def _placed_rule(c):
    return rc.PLACED_ELSEWHERE[c.geometry][0]


@pytest.mark.parametrize("name", [c.name for c in rc.POSITIVE])
def test_fused_block(device, n_cu, name):
    c = rc.BY_NAME[name]
    n_win = c.n_win
    if c.launch is not None:
        n_win = rc.launch_windows(c, n_cu)
        lo, hi = rc.n_local_range(c, n_win, n_cu)
        assert hi == lo + 1 and lo >= int(c.launch), (name, n_cu, n_win, lo, hi)
    else:
        assert 6 * n_win * c.til.tiles < rc.grid(c.c, 1 << 30, n_cu) or n_cu < 256, (name, n_cu)
    _guarded(name, lambda: _positive(device, c, n_win))


def _negative(device, c):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    b = rc.build(c)
    device.set_fuse_resblock(True)
    model = HipModel(device, b.prog)
    failures = []
    try:
        assert model.precision == "f16x3", model.describe()
        assert "fused residual block" not in model.describe(), (c.neg, model.describe())
        taps = Taps(model, b.ids, 0)
        for i in b.extra + [b.conv1, b.conv2]:
            _check_op(taps, i, f"{c.name} op {i}", failures)
            assert not taps.variant[i] & L.TAP_FUSED_RESBLOCK, (c.name, i, hex(taps.variant[i]))
        assert not failures, "\n".join(failures)
    finally:
        model.close()


@pytest.mark.parametrize("name", [c.name for c in rc.NEGATIVE])
def test_not_fused(device, name):
    c = rc.BY_NAME[name]
    _guarded(name, lambda: _negative(device, c))


def _guard(device, c):
    from jaeger_amd.engine import HipModel
    b = rc.build(c)
    device.set_fuse_resblock(True)
    model = HipModel(device, b.prog)
    exact = HipModel(device, b.prog)
    try:
        assert model.precision == "f16x3" and "fused residual block" in _conv_line(model, b.conv2), model.describe()
        got = model.forward(b.ids)
        assert model.precision == "f32", f"{c.name}: the range guard did not trip"
        exact.set_precision("f32")
        want = exact.forward(b.ids)
        assert set(got) == set(want) and "prediction" in got and "embedding" in got
        for key in want:
            assert np.isfinite(want[key]).all(), key
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{c.name}: {key}")
    finally:
        model.close()
        exact.close()


@pytest.mark.parametrize("name", [c.name for c in rc.GUARD])
def test_range_guard(device, name):
    c = rc.BY_NAME[name]
    _guarded(name, lambda: _guard(device, c))
