"""The exact-f32 conv and the layer norm on the GPU, one op at a time: every tile shape, width, row length and channel pass of
``conv_f32_kernel`` and both quad slots of ``layernorm_kernel`` (cases: tests/f32_conv_cases.py; the CPU tier,
tests/test_f32_conv_reference.py, pins the launcher's choices to the source, shows a float32 emulation of the kernels 4 x inside
the bounds on every case and every mutation of them 8 x outside on some case).

Per case, with ``set_precision("f32")`` and the fused residual blocks off:

* the target's tapped tensor against oracle/ops.run_op in float64 from the op's own tapped inputs, with op_cases.check and its
  constants unchanged; a conv reports TAP_EXACT_F32; the first-layer convs that feed it (exact-f32 convs of the case's own
  ``cin`` outputs) are checked the same way;
* the MASK op the target writes under, bit for bit;
* every ``nmd`` vector against the float64 finish of the reference's tap tensors under the GPU's own mask (``nmd_bounds`` of
  tests/test_conv_instance_reference.py);
* one JG_PROF_MFMA_F32 launch per conv and forward;
* where the case names ``chunk=2``: the tapped tensor and the outputs bit-identical to one launch group.

No test here provokes a fault: every program is one the library accepts, or one it refuses on the host.  A failure of the HIP
runtime ends the session (``pytest.exit``): nothing more runs on the device after a fault.
"""
import faulthandler
import time

import numpy as np
import pytest

import f32_conv_cases as fc
import op_cases as oc
from test_conv_instance_reference import nmd_bounds
from test_gpu_op_taps import Taps

pytestmark = pytest.mark.gpu

_ROWS = []          # (kind, label, worst err/bound, rms err/M, worst err/M)
_T0 = [None]


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    d.set_fuse_resblock(False)
    _T0[0] = time.time()
    yield d
    d.set_fuse_resblock(True)
    print("\nexact-f32 conv / layer norm margins (worst err/bound <= 1; rms err/M <= %.3g):" % oc.RMS_BOUND)
    for kind in ("conv", "feeder", "ln", "eltwise", "nmd"):
        rows = [r for r in _ROWS if r[0] == kind]
        if not rows:
            continue
        print("  %-8s %3d checks: worst err/bound %.3g, worst rms err/M %.3g (%.3g of its bound)" %
              (kind, len(rows), max(r[2] for r in rows), max(r[3] for r in rows), max(r[5] for r in rows)))
        for r in sorted(rows, key=lambda r: -r[2])[:4]:
            print("      %-52s worst %8.3g  rms err/M %9.3g  worst err/M %9.3g" % (r[1], r[2], r[3], r[4]))
    print("  %.1f s" % (time.time() - _T0[0]))
    d.close()


def _record(kind, label, res, rms_bound=oc.RMS_BOUND):
    _ROWS.append((kind, label, res.worst, res.rms, res.worst_m, res.rms / rms_bound))


def _guard(name, exc):
    """A HIP call failed (a fault, a lost device): nothing more runs on the device in this session.  A refusal of the library
    itself - an unsupported or invalid program - is a finding and fails this test alone."""
    from jaeger_amd import _lib as L
    if f"failed ({L.JG_ERR_HIP})" in str(exc):
        pytest.exit(f"{name}: {exc}", returncode=3)


def _check_tensor(kind, model, taps, i, label, failures):
    from oracle import ops
    st = taps.state(i)                      # (taps the producers first: the last tapped forward below is op i's own)
    got = model.tap(i, taps.ids, chunk=taps.chunk)
    taps.cache[i], taps.variant[i] = got, model.tap_variant()
    ref = ops.run_op(taps.prog, i, st)
    assert got.shape == ref.out.shape, (label, got.shape, ref.out.shape)
    res = oc.check(got, ref.out, ref.M)
    _record(kind, label, res)
    if not (np.isfinite(got).all() and res.ok):
        failures.append(res.report(label))
    return got, ref, st


def _check_nmd(model, b, chunk, ref, st, label, failures):
    from oracle import ops
    prog = b.prog
    got = model.forward(b.ids, chunk=chunk, want=("nmd",))["nmd"]
    fin = ops.State(st.ids, mask=dict(st.mask))
    fin.part.update(ref.taps)
    fin.part_M.update(ref.taps_M)
    gamma, rms_bound = nmd_bounds(ref.out.shape[1] * ref.out.shape[2])
    for i in b.finals:
        op = prog.ops[i]
        r = ops.run_op(prog, i, fin)
        res = oc.check(got[:, None, None, op.vec_off:op.vec_off + op.cout], r.out[:, None, None, :], r.M[:, None, None, :], gamma=gamma)
        _record("nmd", f"{label} nmd op {i}", res, rms_bound)
        if res.n_bad or res.rms > rms_bound or not np.isfinite(got).all():
            failures.append(res.report(f"{label} nmd op {i} (gamma {gamma:.3g}, rms bound {rms_bound:.3g})"))


def _check_mask(taps, b):
    from oracle import ops
    if b.mask_op is None:
        return
    got = taps.get(b.mask_op)
    ref = ops.run_op(b.prog, b.mask_op, taps.state(b.mask_op))
    np.testing.assert_array_equal(got, ref.out, err_msg=f"mask op {b.mask_op}")


def _launches(device, model, ids):
    """JG_PROF_MFMA_F32 launches of one forward in one launch group."""
    device.profile_enable(True)
    try:
        n0 = device.profile_read()["mfma_f32"]["launches"]
        out = model.forward(ids)
        return device.profile_read()["mfma_f32"]["launches"] - n0, out
    finally:
        device.profile_enable(False)


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_conv_case(device, name):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    c = fc.BY_NAME[name]
    b = fc.build(c)
    failures = []
    model = None
    try:
        model = HipModel(device, b.prog)
        model.set_precision("f32")
        taps = Taps(model, b.ids, c.chunk)
        for i in b.feeders:
            _check_tensor("feeder", model, taps, i, f"{name} feeder op {i}", failures)
            assert taps.variant[i] & L.TAP_EXACT_F32, (name, i, taps.variant[i])
        _check_mask(taps, b)
        got, ref, st = _check_tensor("conv", model, taps, b.target, name, failures)
        assert taps.variant[b.target] & L.TAP_EXACT_F32 and not taps.variant[b.target] & L.TAP_F16S, (name, taps.variant[b.target])
        assert got.shape[2:] == (c.l_out, c.cout)
        if b.finals:
            _check_nmd(model, b, c.chunk, ref, st, name, failures)
        n, whole = _launches(device, model, b.ids)
        assert n == len(b.feeders) + 1, (name, n)
        assert all(np.isfinite(v).all() for v in whole.values())
        if c.chunk:
            one = model.tap(b.target, b.ids, chunk=0)
            np.testing.assert_array_equal(got, one, err_msg=f"{name}: chunk={c.chunk} against one launch group")
            parts = model.forward(b.ids, chunk=c.chunk)
            for k in whole:
                np.testing.assert_array_equal(parts[k], whole[k], err_msg=f"{name} {k}: chunk={c.chunk}")
        assert not failures, "\n".join(failures)
    except L.JaegerHipError as exc:
        _guard(name, exc)
        raise
    finally:
        if model is not None:
            model.close()


@pytest.mark.parametrize("name", [c.name for c in fc.LN_CASES])
def test_layernorm_case(device, name):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    c = fc.LN_BY_NAME[name]
    b = fc.build_ln(c)
    failures = []
    model = None
    try:
        model = HipModel(device, b.prog)
        model.set_precision("f32")
        taps = Taps(model, b.ids, 0)
        _check_mask(taps, b)
        got, ref, st = _check_tensor("ln" if c.is_ln else "eltwise", model, taps, b.target, name, failures)
        assert got.shape[2:] == (c.l, c.c)
        if b.finals:
            _check_nmd(model, b, 0, ref, st, name, failures)
        assert not failures, "\n".join(failures)
    except L.JaegerHipError as exc:
        _guard(name, exc)
        raise
    finally:
        if model is not None:
            model.close()


def test_bad_widths_are_refused_at_model_creation(device):
    """A conv whose cin or cout is no multiple of 4, an element-wise op of such a width and a layer norm above 512 channels
    are refused by jg_model_create with the reason (the launchers' own checks would stop the first forward half way); a model
    created afterwards runs."""
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel

    def refused(prog, word):
        with pytest.raises(L.JaegerHipError, match=word):
            HipModel(device, prog).close()

    try:
        refused(fc.build(fc.Case("bad-cout", cout=30)).prog, r"op \d+: conv of 32 -> 30 channels \(both must be multiples of 4")
        refused(fc.build(fc.Case("bad-cin", first=True, cin=6)).prog, r"op \d+: conv of 6 -> 32 channels \(both must be multiples of 4")
        refused(fc.build(fc.Case("bad-feed", cin=30)).prog, r"op \d+: conv of 8 -> 30 channels")
        bad = fc.build_ln(fc.LnCase("bad-elt", 32, 5, "bn_act"))
        op = L.JgOp.from_buffer_copy(bad.prog.ops[bad.target])
        op.cout = 30
        bad.prog.ops[bad.target] = op
        refused(bad.prog, r"op \d+: element-wise op of 30 channels \(a multiple of 4")
        refused(fc.build_ln(fc.LnCase("bad-ln", 516, 5)).prog, r"op \d+: layer norm over 516 channels \(up to 512")
        good = fc.build_ln(fc.LnCase("good-bn", 516, 5, "bn_act"))          # (a plain element-wise op may be that wide)
        for b in (good, fc.build(fc.BY_NAME["cout32-bn32"])):
            model = HipModel(device, b.prog)
            try:
                model.set_precision("f32")
                out = model.forward(b.ids)
                assert np.isfinite(out["prediction"]).all() and out["prediction"].shape == (b.ids.shape[0], 2)
            finally:
                model.close()
    except L.JaegerHipError as exc:
        _guard("refusals", exc)
        raise
