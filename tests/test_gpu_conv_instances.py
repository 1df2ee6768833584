"""Every compiled instance of the split-f16 conv template against the float64 op reference, on the GPU.

One case per instance (tests/conv_instance_cases.py; its CPU tier, tests/test_conv_instance_reference.py, pins the census to
the source text and shows that every stage of every case is visible in the bounds).  Per case:

* the instance the library reports for the target conv (JG_MSTAT_TAP_INSTANCE: part, K, EP, FLAT, CW, TANH, and the run-time
  stage bits of the JG_EP_RUNTIME pattern) is the one the case exists for, not flagged mixed - the tiling is asserted through
  it, never assumed;
* the tapped tensor against oracle/ops.run_op in float64 from the op's own tapped inputs, with op_cases.check and its
  constants (GAMMA, RMS_BOUND, REL, FLOOR) unchanged; a store-free conv through ``embedding`` (test_gpu_op_taps._check_pool_fused);
* the ``nmd`` vector of every NMD tap against the float64 finish of the reference's tap tensors under the GPU's own mask
  (bound: ``nmd_bounds`` of the CPU module - the conv's GAMMA plus the f32 sum over the positions).

A case the placement must refuse (a DyT pattern with another activation than the tanh-GELU) reports exact f32; the nearest
accepted program of each unreachable instance lands on the instance the census names; one forward whose launch groups take
different tilings reports "mixed" and passes over all windows.
"""
import time

import pytest

import conv_instance_cases as cc
import op_cases as oc
from test_conv_instance_reference import nmd_bounds
from test_gpu_op_taps import Taps, _check_pool_fused

pytestmark = pytest.mark.gpu

_TABLE = []
_SEEN = set()
_T0 = [None]


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    d.set_fuse_resblock(False)          # (a 32- / 64-channel ACT1 conv in front of an ADD + ACT1 one would run as one fused block)
    _T0[0] = time.time()
    yield d
    d.set_fuse_resblock(True)
    print("\nper-instance margins (worst err/bound <= 1; rms err/M <= %.3g):" % oc.RMS_BOUND)
    for row in _TABLE:
        print("  " + row)
    rows = [r for r in _STATS if r[0] == "conv"]
    if rows:
        print("census: %d instances asserted by identity, worst err/bound %.3g, worst rms err/M %.3g; nmd vectors: worst err/bound %.3g; "
              "%.1f s" % (len(_SEEN), max(r[1] for r in rows), max(r[2] for r in rows),
                          max([r[1] for r in _STATS if r[0] == "nmd"] or [0.0]), time.time() - _T0[0]))
    d.close()


_STATS = []


def _record(label, kind, res):
    _STATS.append((kind, res.worst, res.rms))
    _TABLE.append(f"{label:78s} worst {res.worst:8.3g}  rms err/M {res.rms:9.3g}  worst err/M {res.worst_m:9.3g}")


def _as_instance(d):
    return None if d is None else cc.Instance(d["part"], d["k"], d["ep"], d["flat"], d["cw"], d["tanh"])


def _check_conv(model, taps, i, label, failures):
    """Conv op i from its producers' taps; returns (reported instance dict, float64 reference)."""
    from jaeger_amd import _lib as L
    from oracle import ops
    prog = taps.prog
    st = taps.state(i)                      # (taps the producers first: the last tapped forward below is op i's own)
    got = model.tap(i, taps.ids, chunk=taps.chunk)
    variant, inst = model.tap_variant(), model.tap_instance()
    taps.cache[i], taps.variant[i] = got, variant
    ref = ops.run_op(prog, i, st)
    out, M = ref.out, ref.M
    if variant & L.TAP_PHASE_SPLIT:         # stored times its mask for the stride-2 readers
        om = st.mask[prog.ops[i].out_mask][..., None]
        out, M = out * om, M * om
    res = oc.check(got, out, M, f16s=bool(variant & L.TAP_F16S))
    _record(label, "conv", res)
    if not res.ok:
        failures.append(res.report(label))
    return inst, variant, ref, st


def _check_nmd(model, b, c, ref, st, label, failures):
    from oracle import ops
    prog = b.prog
    got = model.forward(b.ids, chunk=c.chunk, want=("nmd",))["nmd"]
    fin = ops.State(st.ids, mask=dict(st.mask))
    fin.part.update(ref.taps)
    fin.part_M.update(ref.taps_M)
    n_pos = ref.out.shape[1] * ref.out.shape[2]
    gamma, rms_bound = nmd_bounds(n_pos)
    for i, _ in b.finals:
        op = prog.ops[i]
        r = ops.run_op(prog, i, fin)
        res = oc.check(got[:, None, None, op.vec_off:op.vec_off + op.cout], r.out[:, None, None, :], r.M[:, None, None, :], gamma=gamma)
        _record(f"{label} nmd op {i}", "nmd", res)
        if res.n_bad or res.rms > rms_bound:
            failures.append(res.report(f"{label} nmd op {i} (gamma {gamma:.3g}, rms bound {rms_bound:.3g})"))


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_instance(device, name):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    from oracle import ops
    c = cc.BY_NAME[name]
    b = cc.build(c)
    model = HipModel(device, b.prog)
    failures = []
    try:
        assert model.precision == "f16x3", model.describe()
        taps = Taps(model, b.ids, c.chunk)
        if c.store == "free":
            # nothing is stored: tap an op in front of the target (its instance is recorded all the same), then the pooled output
            with pytest.raises(L.JaegerHipError, match="store-free"):
                model.tap(b.target, b.ids)
            taps.get(b.target - 1)                                  # (the mask op the target writes under)
            inst = model.tap_instance(op=b.target)
            _check_pool_fused(model, taps, b.target, name, failures)
            st = taps.state(b.target)
            ref = ops.run_op(b.prog, b.target, st)
        else:
            inst, variant, ref, st = _check_conv(model, taps, b.target, name, failures)
            if c.want is None:
                assert inst is None and variant & L.TAP_EXACT_F32, (inst, variant, model.describe())
                assert "not one of the compiled" in model.describe()
            else:
                assert bool(variant & L.TAP_WINDOW_PACKED) == c.want.flat and not variant & L.TAP_EXACT_F32, variant
                assert bool(variant & L.TAP_PHASE_SPLIT) == (c.store == "psplit"), variant
                assert bool(variant & L.TAP_F16S) == (c.store in ("f16s", "psplit")), variant
        if c.want is not None:
            assert inst is not None, model.describe()
            assert _as_instance(inst) == c.want, (inst, c.want)
            assert inst["mixed"] == c.mixed, inst
            if c.want.ep == cc.RT:
                assert inst["ep_rt"] == c.ep_rt, (inst, c.ep_rt)
            if c.mixed:
                assert _as_instance(inst["other"]) == c.want._replace(part=1, flat=False), inst
            _SEEN.add(c.want)
        for r in b.readers:                 # the stride-2 readers of a phase-split store: both read forms
            _check_conv(model, taps, r, f"{name} reader op {r}", failures)
        if b.finals:
            _check_nmd(model, b, c, ref, st, name, failures)
        assert not failures, "\n".join(failures)
    except L.JaegerHipError as exc:
        # a HIP call failed (a fault, a lost device): nothing more runs on the device in this session.  A refusal of the
        # library itself - an unsupported pattern, an invalid program - is a finding and fails this test alone
        if f"failed ({L.JG_ERR_HIP})" in str(exc):
            pytest.exit(f"{name}: {exc}", returncode=3)
        raise
    finally:
        model.close()


def test_every_compiled_instance_was_asserted(device, request):
    """Runs last.  When every case of this module was selected, the instances asserted by identity above are all the
    compiled ones but those the census proves unreachable: a case that failed before its identity check is missing here
    too.  In a narrower selection only the cases that ran can be held to the census."""
    want = cc.compiled_instances() - set(cc.UNREACHABLE)
    selected = sum(1 for item in request.session.items
                   if item.module is request.module and getattr(item, "originalname", "") == "test_instance")
    if selected == len(cc.CASES):
        assert _SEEN == want, sorted(want - _SEEN)
    else:
        assert _SEEN <= want, sorted(_SEEN - want)
