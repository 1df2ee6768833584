"""Per-op parity on the GPU: the tensor every op writes, read back with jg_model_set_tap, against the float64 op reference
(oracle/ops.py) evaluated from exactly the inputs the kernel read (its producers' taps - forwards are bit-repeatable,
tests/test_gpu_parity.py::test_f16x3_repeatable).  Errors therefore do not pile up across layers and the bounds of
tests/op_cases.py (GAMMA, RMS_BOUND; chosen and margined on the CPU by tests/test_op_reference.py) apply op by op, at every
position and channel - where the pooled outputs hide a single wrong position.

MASK and EMBED ops must match bit for bit, MAXPOOL1D too (a maximum of its read-back input).  A conv whose only reader is a
fused max pool stores nothing: it is checked through the ``embedding`` output (the masked maximum of its f64 output); with
JG_OPT_FUSE_RESBLOCK 1 a fused narrow block's output is checked against its two convs evaluated in f64 from the block's input.
Every case asserts the kernel variant (JG_MSTAT_TAP_VARIANT) it is there for.
"""
import numpy as np
import pytest

import op_cases as oc

pytestmark = pytest.mark.gpu

_TABLE = []


@pytest.fixture(scope="module")
def device():
    from jaeger_amd.engine import HipDevice
    d = HipDevice(0)
    yield d
    print("\nper-op margins (worst err/bound <= 1; rms err/M <= %.3g):" % oc.RMS_BOUND)
    for row in _TABLE:
        print("  " + row)
    d.close()


def _writes_act(op, slot):
    from oracle import ops
    return op.kind in (ops.OP_CONV, ops.OP_ELTWISE, ops.OP_MAXPOOL1D, ops.OP_FRAMESUM, ops.OP_EMBED) and op.out_buf == slot


def _producer(prog, i, slot, mask=False):
    from oracle import ops
    for j in range(i - 1, -1, -1):
        o = prog.ops[j]
        if mask and ((o.kind == ops.OP_MASK and o.out_mask == slot) or (o.kind == ops.OP_EMBED and o.out_mask == slot)):
            return j
        if not mask and _writes_act(o, slot):
            return j
    raise AssertionError(f"op {i}: no producer of {'mask' if mask else 'slot'} {slot}")


class Taps:
    """Read-back tensors of one model / precision / chunk, tapped on demand and cached."""

    def __init__(self, model, ids, chunk):
        self.model, self.ids, self.chunk = model, ids, chunk
        self.prog = model.program
        self.cache, self.variant = {}, {}

    def get(self, i):
        if i not in self.cache:
            self.cache[i] = self.model.tap(i, self.ids, chunk=self.chunk)
            self.variant[i] = self.model.tap_variant()
        return self.cache[i]

    def mask(self, i, slot):
        """Mask slot ``slot`` as op i reads it."""
        from oracle import ops
        if slot in (ops.BUF_NONE, ops.BUF_IDS):
            return None
        j = _producer(self.prog, i, slot, mask=True)
        if self.prog.ops[j].kind == ops.OP_EMBED:
            return (self.ids != 0).astype(np.uint8)
        return self.get(j)

    def state(self, i, skip=()):
        """The inputs of op i from its producers' taps (slots in ``skip`` are left out)."""
        from oracle import ops
        op = self.prog.ops[i]
        st = ops.State(ops.program_rows(self.prog, self.ids))
        bufs = [op.in_buf] + [op.stages[s].arg for s in range(op.n_stages) if op.stages[s].kind == ops.ST_ADD]
        for b in bufs:
            if b >= 0 and b not in skip:
                st.act[b] = self.get(_producer(self.prog, i, b))
        masks = () if op.kind == ops.OP_EMBED else (op.in_mask,) if op.kind == ops.OP_MASK else (op.in_mask, op.out_mask)
        for m in masks:
            mk = self.mask(i, m)
            if mk is not None:
                st.mask[m] = mk
        return st


def _record(label, res):
    _TABLE.append(f"{label:58s} worst {res.worst:8.3g}  rms err/M {res.rms:9.3g}  worst err/M {res.worst_m:9.3g}")


def _check_model(dev, name, l, precision, chunk=0, fuse=True, expect=0, n_win=12, prog=None):
    """Every tappable op of the model, checked; ``expect``: variant bits some op must show.  Returns {op index: variant bits}
    of the ops checked through their own tap and {op index: "pooled" / "fused"} of those checked another way."""
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    from oracle import ops
    if prog is None:
        _, _, prog = oc.compile_model(name)
    dev.set_fuse_resblock(fuse)
    model = HipModel(dev, prog)
    try:
        model.set_precision(precision)
        ids = oc.edge_ids(l, n_win=n_win, vocab=prog.vocab)
        taps = Taps(model, ids, chunk)
        seen = 0
        failures = []
        checked, other = {}, {}
        for i, op in enumerate(prog.ops):
            label = f"{name} l={l} {precision}{' chunk=%d' % chunk if chunk else ''}{'' if fuse else ' nofuse'} op {i}"
            if op.kind not in (ops.OP_CONV, ops.OP_MASK, ops.OP_ELTWISE, ops.OP_EMBED, ops.OP_MAXPOOL1D, ops.OP_FRAMESUM):
                continue
            try:
                got = taps.get(i)
            except L.JaegerHipError as exc:
                msg = str(exc)
                assert op.kind == ops.OP_CONV and precision == "f16x3", (label, msg)
                if "store-free" in msg:
                    _check_pool_fused(model, taps, i, label, failures)
                    other[i] = "pooled"
                elif "fused residual block" in msg:
                    assert fuse and "JG_OPT_FUSE_RESBLOCK 0" in msg, msg
                    other[i] = "fused"
                else:
                    raise
                continue
            seen |= taps.variant[i]
            checked[i] = taps.variant[i]
            if op.kind == ops.OP_CONV and precision == "f32":
                assert taps.variant[i] & L.TAP_EXACT_F32, (label, taps.variant[i])
            if op.kind == ops.OP_CONV and taps.variant[i] & L.TAP_FUSED_RESBLOCK:
                # conv1 of the block never exists: both convs in f64 from the block's input
                st, ref = _fused_block_ref(prog, taps, i)
            else:
                st = taps.state(i)
                ref = ops.run_op(prog, i, st)
            if op.kind == ops.OP_MASK:
                np.testing.assert_array_equal(got, ref.out, err_msg=label)
                continue
            if op.kind == ops.OP_EMBED:
                np.testing.assert_array_equal(got, ref.out.astype(np.float32), err_msg=label)
                continue
            if op.kind == ops.OP_MAXPOOL1D:
                np.testing.assert_array_equal(got, ref.out.astype(np.float32), err_msg=label)
                continue
            out, M = ref.out, ref.M
            if taps.variant[i] & L.TAP_PHASE_SPLIT:           # stored times its mask for the stride-2 readers
                om = st.mask[op.out_mask][..., None]
                out, M = out * om, M * om
            res = oc.check(got, out, M, f16s=bool(taps.variant[i] & L.TAP_F16S))
            _record(label, res)
            if not res.ok:
                failures.append(res.report(label))
        assert not failures, "\n".join(failures)
        assert seen & expect == expect, (name, precision, f"variant bits seen {seen:#x}, expected {expect:#x}")
        if precision == "f16x3":          # the variant bits agree with the placement: only convs it leaves on f32 report f32
            pl = model.placement()
            n_f32 = sum(1 for j, v in checked.items() if prog.ops[j].kind == ops.OP_CONV and v & L.TAP_EXACT_F32)
            assert n_f32 == pl["convs"] - pl["convs_f16x3"], (name, n_f32, pl, model.describe())
        return checked, other
    finally:
        model.close()
        dev.set_fuse_resblock(True)


def _fused_block_ref(prog, taps, i):
    from oracle import ops
    op = prog.ops[i]
    first = _producer(prog, i, op.in_buf)
    st1 = taps.state(first)
    r1 = ops.run_op(prog, first, st1)
    st = taps.state(i, skip=(op.in_buf,))
    st.act[op.in_buf] = r1.out
    st.M[op.in_buf] = r1.M
    return st, ops.run_op(prog, i, st)


def _check_pool_fused(model, taps, i, label, failures):
    """A store-free conv: its masked max pool (the embedding output) against the f64 masked max of its output."""
    from oracle import ops
    prog = taps.prog
    op = prog.ops[i]
    pool = next(j for j in range(i + 1, len(prog.ops)) if prog.ops[j].kind == ops.OP_POOL and prog.ops[j].in_buf == op.out_buf
                and prog.ops[j].in_mask == op.out_mask)
    po = prog.ops[pool]
    assert po.out_vec == ops.VEC_EMBEDDING, "a fused pool that does not write the embedding output"
    st = taps.state(i)
    ref = ops.run_op(prog, i, st)
    st.act[prog.ops[i].out_buf] = ref.out
    pooled = ops.run_op(prog, pool, st).out
    st.act[prog.ops[i].out_buf] = ref.M
    pooled_m = ops.run_op(prog, pool, st).out
    got = model.forward(taps.ids, chunk=taps.chunk, want=("embedding",))["embedding"][:, po.vec_off:po.vec_off + po.cout]
    res = oc.check(got[:, None, None, :], pooled[:, None, None, :], pooled_m[:, None, None, :])
    _record(label + " (pooled)", res)
    if not res.ok:
        failures.append(res.report(label + " (pooled)"))


# ---- the case matrix ----------------------------------------------------------------------------------------------
def _kind_ops(prog, kind, pred=lambda op: True):
    return [i for i, op in enumerate(prog.ops) if op.kind == kind and pred(op)]


def _f32_convs(checked, prog):
    """Every conv checked, and every one on the exact-f32 kernel."""
    from jaeger_amd import _lib as L
    from oracle import ops
    convs = _kind_ops(prog, ops.OP_CONV)
    assert set(convs) <= set(checked), sorted(set(convs) - set(checked))
    assert all(checked[i] & L.TAP_EXACT_F32 and not checked[i] & L.TAP_F16S for i in convs)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("chunk", [0, 4])
def test_brain_1500(device, precision, chunk):
    """Table-lookup first conv, k = 5 / d = 3 at 128 channels, fused epilogues with ADD / NMD, the store-free max-pool conv
    (through the embedding); chunk = 4: the readback assembled across three launch groups of the 12 windows."""
    from jaeger_amd import _lib as L
    from oracle import ops
    _, _, prog = oc.compile_model("brain")
    checked, other = _check_model(device, "brain", 500, precision, chunk=chunk, prog=prog)
    first = _kind_ops(prog, ops.OP_CONV)[0]
    assert len(_kind_ops(prog, ops.OP_MASK)) == 13 and set(_kind_ops(prog, ops.OP_MASK)) <= set(checked)
    if precision == "f32":
        _f32_convs(checked, prog)
        return
    assert checked[first] & L.TAP_TABLE_LOOKUP, checked[first]
    assert list(other.values()) == ["pooled"], other
    assert sum(1 for i, v in checked.items() if prog.ops[i].kind == ops.OP_CONV and v & L.TAP_F16S) >= 10


@pytest.mark.parametrize("l", [665, 832])
def test_brain_window_packed(device, l):
    """665 and 832 codons per frame: the frames fill their own tiles badly and the convs take window-packed tiles (split-f16
    only: the exact-f32 kernel has no such tiling)."""
    from jaeger_amd import _lib as L
    _check_model(device, "brain", l, "f16x3", n_win=8, expect=L.TAP_WINDOW_PACKED | L.TAP_F16S)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_zeus_dyt(device, precision):
    """DyT epilogues with and without the mask (zeus with its last residual stack unmasked)."""
    from oracle import ops
    _, _, prog = oc.compile_model("zeus_mixed")
    checked, _ = _check_model(device, "zeus_mixed", 500, precision, prog=prog)
    dyt = {prog.ops[i].stages[q].arg for i in checked for q in range(prog.ops[i].n_stages)
           if prog.ops[i].kind == ops.OP_CONV and prog.ops[i].stages[q].kind == ops.ST_DYT}
    assert dyt == {0, 1}, dyt
    if precision == "f32":
        _f32_convs(checked, prog)


@pytest.mark.parametrize("fuse", [False, True])
def test_pyramid(device, fuse):
    """Stride-2 phase-split stores and both phase-split read forms, 32 / 64 narrow tiles, 256-wide convs, 1x1 bypasses;
    fuse: the narrow blocks as one launch, checked against both convs from the block's input."""
    from jaeger_amd import _lib as L
    from oracle import ops
    _, _, prog = oc.compile_model("pyramid")
    expect = L.TAP_PHASE_SPLIT | L.TAP_NARROW | L.TAP_F16S | (L.TAP_FUSED_RESBLOCK if fuse else 0)
    checked, other = _check_model(device, "pyramid", 665, "f16x3", fuse=fuse, n_win=8, expect=expect, prog=prog)
    convs = _kind_ops(prog, ops.OP_CONV)
    assert set(convs) <= set(checked) | set(other)
    assert ("fused" in other.values()) == fuse
    assert any(prog.ops[i].cout == 256 for i in convs if i in checked)
    assert any(prog.ops[i].k == 1 and prog.ops[i].stride == 2 for i in convs if i in checked)


@pytest.mark.parametrize("name,precision", [("pyramid", "f32"), ("pyramid_k7", "f16x3"), ("pyramid_k7", "f32"),
                                            ("pyramid_k9", "f16x3"), ("pyramid_k9", "f32")])
def test_pyramid_taps_and_arithmetic(device, name, precision):
    """The pyramid with 5- (f32 leg), 7- and 9-tap blocks: the run-time-geometry split-f16 instantiations (narrow tiles; the
    7- / 9-tap stride-2 convs evaluated at stride 1 with every second output dropped - only 5-tap ones read phase-split
    tensors) and the exact-f32 kernel on the same shapes."""
    from jaeger_amd import _lib as L
    _, _, prog = oc.compile_model(name)
    expect = L.TAP_NARROW | L.TAP_F16S if precision == "f16x3" else L.TAP_EXACT_F32
    checked, _ = _check_model(device, name, 665, precision, n_win=6, expect=expect, prog=prog)
    if precision == "f32":
        _f32_convs(checked, prog)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_baseline500_layer_by_layer(device, precision):
    """Rows too long for the fused small-window kernel: the narrow split-f16 kernels, 3-tap convs as tap-masked 5-tap ones."""
    from jaeger_amd import _lib as L
    from oracle import ops
    _, _, prog = oc.compile_model("baseline500")
    checked, _ = _check_model(device, "baseline500", 500, precision, prog=prog,
                              expect=L.TAP_NARROW | L.TAP_F16S if precision == "f16x3" else 0)
    assert any(prog.ops[i].k == 3 for i in _kind_ops(prog, ops.OP_CONV) if i in checked)
    if precision == "f32":
        _f32_convs(checked, prog)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["brain_ln", "brain_majority", "brain_strict"])
def test_layernorm_and_mask_modes(device, name, precision):
    """The LayerNorm element-wise op (LN leading its stage list) and the majority / strict mask rules, bit for bit."""
    from oracle import ops
    _, _, prog = oc.compile_model(name)
    checked, _ = _check_model(device, name, 500, precision, n_win=8, prog=prog)
    if name == "brain_ln":
        ln = _kind_ops(prog, ops.OP_ELTWISE, lambda op: op.n_stages > 0 and op.stages[0].kind == ops.ST_LN)
        assert len(ln) == 12 and set(ln) <= set(checked)
    else:
        mode = ops.MASK_MAJORITY if name.endswith("majority") else ops.MASK_STRICT
        masks = _kind_ops(prog, ops.OP_MASK, lambda op: op.mask_mode == mode)     # (the first conv's: blocks use "any")
        assert len(masks) >= 1 and set(masks) <= set(checked)
    if precision == "f32":
        _f32_convs(checked, prog)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_dicodon_positional_embeddings(device, precision):
    """The EMBED op: 16-bit ids gathered and the position rows added, bit for bit; the convs behind it."""
    from oracle import ops
    _, _, prog = oc.compile_model("baseline500_dicodon_pos")
    checked, _ = _check_model(device, "baseline500_dicodon_pos", 300, precision, prog=prog)
    emb = _kind_ops(prog, ops.OP_EMBED, lambda op: op.w_off >= 0)
    assert prog.vocab > 256 and len(emb) == 1 and emb[0] in checked
    if precision == "f32":
        _f32_convs(checked, prog)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_legacy_tower_real_weights(device, precision):
    """The legacy tower on its real weights: MAXPOOL1D on F16S tensors in split-f16 (on f32 ones in exact f32), FRAMESUM,
    exact-erf GELU epilogues at real dynamic ranges."""
    from conftest import GOLDEN

    from jaeger_amd import _lib as L
    from jaeger_amd import legacy
    from oracle import ops
    w = legacy.load_legacy_h5(GOLDEN / "legacy_data" / "models" / "default" / "WRes_1024.h5")
    prog = legacy.compile_legacy(w)
    checked, _ = _check_model(device, "legacy", 665, precision, n_win=6, prog=prog)
    pools = _kind_ops(prog, ops.OP_MAXPOOL1D)
    assert len(pools) == 2 and set(pools) <= set(checked)
    assert _kind_ops(prog, ops.OP_FRAMESUM)[0] in checked
    if precision == "f16x3":
        assert all(checked[i] & L.TAP_F16S for i in pools), {i: checked[i] for i in pools}
    else:
        assert not any(checked[i] & L.TAP_F16S for i in pools)
        _f32_convs(checked, prog)


def test_refusals_and_untapped_forward_unchanged(device):
    """With the tap off again a forward is bit-identical to one before any tap, and launches as many convs; pool / dense
    ops and the streamed path refuse a tap."""
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import HipModel
    from oracle import ops
    _, _, prog = oc.compile_model("brain")
    model = HipModel(device, prog)
    ids = oc.edge_ids(500, n_win=6)
    try:
        device.profile_enable(True)
        before = model.forward(ids)
        n0 = device.profile_read()["conv_launches"]
        model.tap(3, ids)
        pool = next(i for i, op in enumerate(prog.ops) if op.kind == ops.OP_POOL)
        buf = np.zeros(16, np.float32)
        assert model.lib.jg_model_set_tap(model.handle, pool, buf.ctypes.data, buf.nbytes) == L.JG_ERR_UNSUPPORTED
        assert "outputs already" in model.lib.jg_last_error().decode()
        # the streamed / fused path refuses to run while a tap is set (before it touches any buffer)
        tapped = np.zeros(16 * 6 * 500 * 128, np.float32)
        L.check(model.lib.jg_model_set_tap(model.handle, 3, tapped.ctypes.data, tapped.nbytes))
        bases = np.frombuffer(b"ACGT" * 400, np.uint8).copy()
        with pytest.raises(L.JaegerHipError, match="a tap is set"):
            model.predict_windows(bases, bases.size, np.zeros(1, np.int64), np.full(1, 1500, np.int32), 1, 1500,
                                  np.zeros(65, np.uint8))
        assert model.lib.jg_model_set_tap(model.handle, -1, None, 0) == L.JG_OK
        n1 = device.profile_read()["conv_launches"]
        after = model.forward(ids)
        n2 = device.profile_read()["conv_launches"]
        device.profile_enable(False)
        for k in before:
            np.testing.assert_array_equal(before[k], after[k])
        assert n2 - n1 == n0, (n0, n1, n2)
    finally:
        model.close()
