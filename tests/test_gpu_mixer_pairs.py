"""The row-mixer layers next to each other on the GPU (the CPU tier is tests/test_mixer_reference.py, the reference side
tests/mixer_reference.py).

Every ordered pair of the seven row-mixer layers the compiler accepts (46 of 49) at 32 channels, thirteen wide hand-overs
(a width-changing first layer 32 -> 64 in front of each other kind at 64 channels; a bilstm 32 -> 128 into a multi-scale
conv 128 -> 32, so that one slot holds 128-wide and 32-wide rows in one forward) and two chains of all seven layers, each
through ``HipModel.forward`` on three kinds of windows (``full``, ``long_n``, ``empty_row``; every generator with the grow of
the convs in front).  Three windows of 165 codon ids are 18 frame rows - the bilstm's 16-row group and a ragged group of 2.
The 7-tap 'valid' conv in front leaves the mixers rows of 159 positions: local-attention tiles of 80 + 79, length-attention
tiles of 128 + 31, hyena and multi-scale tiles of 64 + 64 + 31.

Per case and window kind:

* logits, embedding and NMD against ``mixer_reference.forward`` at the project's gate (``test_gpu_hyena.check_vectors``);
  ``chunk=2`` (launch groups of 2 + 1 windows) bit for bit the same;
* EVERY mixer op of BOTH layers through its own module's ``check_op`` with that module's bounds as they are (4 x the
  emulation's error, exact zeros at dead and masked positions, the MSMASK mask exact).  A frame-attention op has no
  ``check_op`` in tests/test_gpu_frameattn.py - the comparison is written inside its test - so :func:`check_frame_op` here is
  those lines; the element-wise op that closes an axial block goes through ``oracle.ops.run_op`` and ``op_cases.check`` as
  tests/test_gpu_op_taps.py checks every element-wise op;
* behind a local first layer the reference holds 1e3 at dead positions where the engine holds zeros: agreement at the gate
  shows that the second layer reads neither.

The pairs run in the program's default arithmetic (the conv in front is split-f16: the first mixer's producer stores f32 rows
for it), the chains in both.  No test here provokes a fault; every test runs under a watchdog that ends the process if a GPU
call does not return.
"""
import faulthandler

import numpy as np
import pytest

import attention_reference as ar
import bilstm_reference as br
import hyena_reference as hr
import mixer_reference as mx
import multiscale_reference as mr
import op_cases as oc
import test_gpu_axialattn as gpu_axial
import test_gpu_bilstm as gpu_bilstm
import test_gpu_hyena as gpu_hyena
import test_gpu_localattn as gpu_local
import test_gpu_multiscale as gpu_multiscale
from test_gpu_hyena import check_vectors

pytestmark = pytest.mark.gpu

_TABLE = []
PAIRS = [(a, b) for a in mx.KINDS for b in mx.KINDS if (a, b) not in mx.REFUSED]
OP_NAMES = ("frame attention", "local attention", "length attention", "hyena", "bilstm", "multi-scale conv")


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nevery mixer op of the pair, wide and chain models against its restatement on its own input:")
    for row in _TABLE:
        print("  " + row)


@pytest.fixture(scope="module")
def ids_by_kind():
    return {kind: mx.ids_of(kind) for kind in mx.WINDOW_KINDS}


def _moved_row(module):
    """A sibling module's ``check_op`` files its row in that module's table: it belongs in this one."""
    _TABLE.append(module._TABLE.pop())


def check_frame_op(eng, weights, i, prefix, ids, what):
    """A frame-attention op from its own read-back input: the comparison of
    tests/test_gpu_frameattn.py::test_model_outputs_and_attention_op, its bound unchanged."""
    from jaeger_amd import _lib as L
    prog = eng.program
    op = prog.ops[i]
    x = eng.model.tap(mx.producer(prog, i), ids)
    y = eng.model.tap(i, ids)
    bits = eng.model.tap_variant()
    assert bits & L.TAP_EXACT_F32 and not bits & (L.TAP_F16S | L.TAP_PHASE_SPLIT), (what, bits)
    lw = ar.sub_weights(weights, prefix)
    use_ffn = op.arg > 0
    want = ar.apply_stages(ar.cross_frame_attention(x, lw, op.k, use_ffn), prog, op)
    emu = ar.apply_stages(ar.emulate(x, lw, op.k, use_ffn), prog, op, dtype=np.float32)
    b = ar.bounds_from(emu, want)
    e, r = ar.errors(y, want)
    _TABLE.append(f"{what:40s} op {i:2d} frame attention: max {e:.3g} (emulation {b['emu_elem']:.3g}, bound {b['elem']:.3g}), "
                  f"rms {r:.3g} (emulation {b['emu_rms']:.3g}, bound {b['rms']:.3g})")
    print(_TABLE[-1])
    assert np.isfinite(y).all() and e <= b["elem"] and r <= b["rms"], _TABLE[-1]


def check_closing_op(eng, i, ids, what):
    """The element-wise op that closes an axial block (post norm, the add of the block's input, the fused tail) from its
    own read-back inputs: ``oracle.ops.run_op`` under ``op_cases.check``, as tests/test_gpu_op_taps.py holds such ops."""
    from jaeger_amd import _lib as L
    from oracle import ops
    prog = eng.program
    op = prog.ops[i]
    st = ops.State(ops.program_rows(prog, ids))
    st.act[op.in_buf] = eng.model.tap(mx.producer(prog, i), ids)
    for s in range(op.n_stages):
        if op.stages[s].kind == L.ST_ADD:
            st.act[op.stages[s].arg] = eng.model.tap(mx.producer(prog, i, op.stages[s].arg), ids)
    if op.out_mask >= 0:
        writer = next(j for j in range(i - 1, -1, -1) if prog.ops[j].out_mask == op.out_mask and prog.ops[j].kind in (L.OP_MASK, L.OP_MSMASK))
        st.mask[op.out_mask] = eng.model.tap(writer, ids)
    got = eng.model.tap(i, ids)
    ref = ops.run_op(prog, i, st)
    res = oc.check(got, ref.out, ref.M)
    _TABLE.append(f"{what:40s} op {i:2d} closing element-wise op: worst err/bound {res.worst:.3g}, rms err/M {res.rms:.3g} (bound {oc.RMS_BOUND:.3g})")
    print(_TABLE[-1])
    assert res.ok, res.report(f"{what} op {i}")


def check_layers(eng, cfg, weights, layers, ids, what):
    """Every op of every mixer layer; returns the dead positions a local layer left, per layer (0 for the other kinds)."""
    dead_of = []
    for short, prefix, a, idxs in layers:
        n_dead = 0
        if short == "cross":
            check_frame_op(eng, weights, idxs[0], prefix, ids, what)
        elif short == "local":
            for j, i in enumerate(idxs):
                dead, _ = gpu_local.check_op(eng, cfg, weights, i, f"{prefix}/block{j}", ids, what)
                _moved_row(gpu_local)
                n_dead = int(dead.sum())
        elif short == "encoder":
            gpu_axial.check_op(eng.model, weights, idxs[0], prefix, ids, what)
            _moved_row(gpu_axial)
        elif short == "axial":
            for j in range(len(idxs) // 3):
                gpu_axial.check_op(eng.model, weights, idxs[3 * j], f"{prefix}/block{j}/length", ids, what)
                _moved_row(gpu_axial)
                check_frame_op(eng, weights, idxs[3 * j + 1], f"{prefix}/block{j}/frame", ids, what)
                check_closing_op(eng, idxs[3 * j + 2], ids, what)
        elif short == "hyena":
            gpu_hyena.check_op(eng, weights, idxs[0], prefix, hr.params_of(a), ids, what)
            _moved_row(gpu_hyena)
        elif short == "bilstm":
            gpu_bilstm.check_op(eng, weights, idxs[0], prefix, br.params_of(a), ids, what)
            _moved_row(gpu_bilstm)
        else:
            gpu_multiscale.check_op(eng, weights, idxs[-1], prefix, mr.params_of(a), ids, what)
            _moved_row(gpu_multiscale)
        dead_of.append(n_dead)
    return dead_of


def run_model(cfg, what, ids_by_kind, both_arithmetics=False):
    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    weights = mx.random_weights(cfg)
    eng = JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0)
    try:
        assert eng.model.precision == "f16x3", eng.model.precision      # the convs in front have a split-f16 program
        assert eng.model.placement()["convs_f16x3"] >= 1 and not eng.model.placement()["small_fused"]
        prog = eng.program
        layers = mx.layer_ops(cfg, prog)
        slots = [s for op in prog.ops for s in (op.in_buf, op.out_buf, op.in_mask, op.out_mask)]
        assert max(slots) < L.JG_MAX_BUFS                                # no more activation or mask slots than the engine has
        refs = {kind: mx.forward(cfg, weights, ids) for kind, ids in ids_by_kind.items()}      # once, for both arithmetics
        dead_behind_local = 0
        for precision in (["f16x3", "f32"] if both_arithmetics else ["f16x3"]):
            eng.model.set_precision(precision)
            assert eng.model.precision == precision
            for kind, ids in ids_by_kind.items():
                label = f"{what} / {precision} / {kind}"
                got = eng.model.forward(ids)
                errs = check_vectors(label, got, refs[kind])
                print(label, {k: f"{v:.2e}" for k, v in errs.items()})
                split = eng.model.forward(ids, chunk=2)               # launch groups of 2 + 1 windows: bit for bit the same
                for k in got:
                    np.testing.assert_array_equal(got[k], split[k], err_msg=f"{label} {k}: chunk 2")
                dead_of = check_layers(eng, cfg, weights, layers, ids, label)
                if kind == "long_n":
                    dead_behind_local += sum(dead_of[:-1])
        return eng.model.describe(), layers, dead_behind_local
    finally:
        eng.close()


@pytest.mark.parametrize("a, b", PAIRS)
def test_pair(a, b, ids_by_kind):
    """Layer ``a`` directly in front of layer ``b`` at 32 channels, in the program's default arithmetic."""
    _, layers, dead = run_model(mx.pair_cfg(a, b), f"{a} -> {b}", ids_by_kind)
    assert [row[0] for row in layers] == [a, b]
    if a == "local":            # the reference held 1e3 there, the engine zeros: the second layer read neither
        assert dead > 0, "the long invalid run left no dead position behind the first layer"


@pytest.mark.parametrize("a, b", mx.WIDE)
def test_wide_handover(a, b, ids_by_kind):
    """Rows of two widths through the same slots."""
    _, layers, _ = run_model(mx.wide_cfg(a, b), f"wide {a} -> {b}", ids_by_kind)
    assert len(layers) == 2


@pytest.mark.parametrize("name", mx.CHAINS)
def test_chain(name, ids_by_kind):
    """All seven layers in one model, in both arithmetics of the conv stack."""
    cfg = mx.chain_cfg(name)
    text, layers, dead = run_model(cfg, name, ids_by_kind, both_arithmetics=True)
    assert tuple(row[0] for row in layers) == mx.CHAINS[name]
    for word in OP_NAMES:
        assert word in text, (word, text)
    if name == "masked_first":          # (its local layer reads a mask; in the other chain none arrives)
        assert dead > 0
