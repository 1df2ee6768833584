"""The float64 op interpreter (oracle/ops.py) on the CPU tier:

(a) chained from the ids, it computes the oracle's network (oracle/forward.py, oracle/legacy.py) from the compiled program -
    this pins jaeger_amd/program.py (epilogue fusion, slot allocation, BN folded to inv_std, padded kernels, position
    tables, mask ops) far tighter than the GPU gate of 1e-4 does;
(b) the per-op check of tests/test_gpu_op_taps.py passes the split-f16 arithmetic (emulated in numpy) and flags each of the
    bugs a tiled conv kernel typically has.
"""
import copy

import numpy as np
import pytest
import torch

import op_cases as oc

#: (a) bound, relative to the largest |output|.  The program stores inv_std = 1 / sqrt(var + eps) in f32; the reference below
#: is given the variance for which float64 gives that same inv_std, so what is left is float64 rounding and the f32 epsilon
#: of a layer norm (1e-3 stored as 0.0010000000475): measured <= 3e-11 relative (brain_ln), everything else <= 2e-15.
REL_3A = 2e-9

MODELS_3A = ["brain", "zeus", "zeus_mixed", "pyramid", "pyramid_k7", "pyramid_k9", "baseline500", "nmdmerge500", "stacks2", "brain_ln",
             "brain_majority", "brain_strict", "baseline500_dicodon_pos"]


def _f32_inv_std_weights(w: dict, eps: float) -> dict:
    w = dict(w)
    for k in list(w):
        if k.endswith("/moving_variance"):
            inv = (np.float32(1.0) / np.sqrt(w[k].astype(np.float32) + np.float32(eps))).astype(np.float32)
            w[k] = 1.0 / inv.astype(np.float64) ** 2 - eps
    return w


@pytest.mark.parametrize("name", MODELS_3A)
def test_interpreter_computes_the_oracle_network(name):
    from oracle import forward as ofwd
    from oracle import ops
    cfg, w, prog = oc.compile_model(name)
    ids = oc.edge_ids(300, n_win=4, vocab=prog.vocab)
    got = ops.outputs(prog, ids)
    ref = ofwd.forward(cfg, _f32_inv_std_weights(w, 1e-5), ids, dtype=torch.float64)
    assert set(ref) <= set(got), (sorted(ref), sorted(got))
    for k, r in ref.items():
        assert got[k].shape == r.shape, k
        err = float(np.abs(got[k] - r).max())
        scale = max(1.0, float(np.abs(r).max()))
        assert err <= REL_3A * scale, (name, k, err, scale)


def test_interpreter_computes_the_legacy_tower_on_real_weights():
    from conftest import GOLDEN

    from jaeger_amd import legacy
    from oracle import legacy as ol
    from oracle import ops
    w = legacy.load_legacy_h5(GOLDEN / "legacy_data" / "models" / "default" / "WRes_1024.h5")
    prog = legacy.compile_legacy(w)
    ids = np.random.Generator(np.random.PCG64(3)).integers(0, 22, (3, 6, 301)).astype(np.uint8)
    ids[1, :, 200:] = 0
    got = ops.outputs(prog, ids)
    ref = ol.forward(_f32_inv_std_weights(w, legacy.BN_EPS), ids, dtype=torch.float64)   # (returned as f32)
    for k_got, k_ref in (("prediction", "output"), ("embedding", "embedding")):
        err = np.abs(got[k_got] - ref[k_ref])
        assert (err <= 2.0 ** -23 * np.abs(ref[k_ref]) + 1e-9).all(), (k_got, float(err.max()))


def test_mask_ops_follow_the_rules():
    """JG_OP_MASK against a direct count on a hand-made mask: any / majority / strict, SAME and VALID, stride 2, dilation."""
    from oracle import ops
    m = np.array([[[1, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1]]], np.uint8)
    assert ops.mask_rule(m, 3, 1, 1, ops.PAD_SAME, ops.MASK_ANY).tolist() == [[[1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1]]]
    assert ops.mask_rule(m, 3, 1, 1, ops.PAD_SAME, ops.MASK_MAJORITY).tolist() == [[[1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1]]]
    assert ops.mask_rule(m, 3, 1, 1, ops.PAD_SAME, ops.MASK_STRICT).tolist() == [[[0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]]]
    assert ops.mask_rule(m, 3, 1, 1, ops.PAD_VALID, ops.MASK_STRICT).tolist() == [[[0, 0, 0, 0, 0, 1, 0, 0, 0]]]
    assert ops.mask_rule(m, 5, 2, 1, ops.PAD_SAME, ops.MASK_ANY).tolist() == [[[1, 1, 1, 1, 1, 1]]]
    assert ops.mask_rule(m, 3, 1, 3, ops.PAD_SAME, ops.MASK_STRICT).tolist() == [[[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]]


# ---- (b) the checker can fail ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brain_conv2():
    """The second conv of brain's first residual block (k = 5, dilation 3, 128 -> 128, bias + BN + residual add + GELU) on
    rows of 300 codons: its inputs from the float64 program run, its exact output and magnitude."""
    from oracle import ops
    cfg, w, prog = oc.compile_model("brain")
    ids = oc.edge_ids(300, n_win=12, vocab=prog.vocab)
    convs = [i for i, op in enumerate(prog.ops) if op.kind == ops.OP_CONV]
    i = next(c for c in convs if any(prog.ops[c].stages[s].kind == ops.ST_ADD for s in range(prog.ops[c].n_stages)))
    state = ops.State(ops.program_rows(prog, ids))
    for j in range(i):
        ops.apply(prog, j, state, ops.run_op(prog, j, state))
    ref = ops.run_op(prog, i, state)
    return prog, i, state, ref, ids


def _emulated(brain_conv2, **kw):
    prog, i, state, ref, _ = brain_conv2
    return oc.emulate_conv(prog, i, state, **kw)


def _with_stages(prog, i, state, y_lin):
    """The op's epilogue on a (mutated) linear part, in f32 like the emulation, re-split."""
    from oracle import ops
    v, _, _ = ops._stages(prog, prog.ops[i], y_lin, np.zeros_like(y_lin), state)
    return oc.resplit(v.astype(np.float32)).astype(np.float64)


def _linear(prog, i, state):
    from oracle import ops
    op = prog.ops[i]
    x = ops.conv_input(prog, op, state)
    lo, pl = ops.conv_geometry(x.shape[-2], op.k, op.stride, op.dilation, op.padding)
    return ops.shifted_sum(x, ops.conv_weights(prog, op), op.stride, op.dilation, pl, lo)


def _mutations(brain_conv2):
    from oracle import ops
    prog, i, state, ref, ids = brain_conv2
    op = prog.ops[i]
    lin = _linear(prog, i, state)
    muts = {}
    # one tap dropped at one output position: 255, the last of a tile (window 0, frame 0)
    muts["tap dropped at position 255"] = _with_stages(
        prog, i, state, lin - oc.tap_contribution(prog, i, state, 0, rows=slice(0, 1), positions=[255]))
    # the halo of one tap read one position off across the tile edge (output 256 reads positions < 256 through tap 0)
    muts["halo read one position off at the tile edge"] = _with_stages(
        prog, i, state, lin - oc.tap_contribution(prog, i, state, 0, rows=slice(0, 1), positions=[256])
        + oc.tap_contribution(prog, i, state, 0, rows=slice(0, 1), positions=[256], shift=-1))
    # the input mask not applied at one masked position that holds a nonzero value
    m = state.mask[op.in_mask]
    r, f, p = (int(v[0]) for v in np.nonzero(m[:, :, 8:-8] == 0))
    p += 8
    unmasked = copy.copy(state)
    unmasked.mask = dict(state.mask)
    unmasked.mask[op.in_mask] = m.copy()
    unmasked.mask[op.in_mask][r, f, p] = 1
    assert np.abs(state.act[op.in_buf][r, f, p]).max() > 0
    muts["input mask not applied at one position"] = _with_stages(prog, i, state, _linear(prog, i, unmasked))
    # the hi_x lo_w cross term dropped for the whole op
    muts["hi_x lo_w dropped"] = oc.emulate_conv(prog, i, state, drop_cross=True)
    # two neighbouring channels' BN affines swapped
    swapped = copy.copy(prog)
    swapped.blob = prog.blob.copy()
    bn = next(op.stages[s] for s in range(op.n_stages) if op.stages[s].kind == ops.ST_BN)
    for off in (bn.p0, bn.p1, bn.p2, bn.p3):
        swapped.blob[[off + 40, off + 41]] = swapped.blob[[off + 41, off + 40]]
    muts["BN affines of channels 40 and 41 swapped"] = oc.emulate_conv(swapped, i, state)
    # window-packed tiling: the last position of window w taken from window w + 1
    y = oc.emulate_conv(prog, i, state)
    y[8, 5, -1] = y[9, 5, -1]
    muts["last position of window 8 from window 9"] = y
    return muts


def test_checker_passes_the_split_f16_emulation(brain_conv2):
    prog, i, state, ref, _ = brain_conv2
    res = oc.check(_emulated(brain_conv2), ref.out, ref.M, f16s=True)
    print(res.report("emulation"))
    assert res.ok, res.report("emulation")


def test_checker_flags_every_mutation(brain_conv2):
    prog, i, state, ref, _ = brain_conv2
    for what, y in _mutations(brain_conv2).items():
        res = oc.check(y, ref.out, ref.M, f16s=True)
        print(res.report(what))
        assert not res.ok, what


def test_checker_bounds_sit_between_emulation_and_mutations(brain_conv2):
    """The margins the module docstring of tests/op_cases.py states: the element bound >= 4x above the largest emulated
    legitimate error and >= 8x below the smallest mutation error; the same for the RMS bound and the emulation."""
    prog, i, state, ref, _ = brain_conv2
    emu = oc.check(_emulated(brain_conv2), ref.out, ref.M, f16s=True)
    assert emu.worst * 4 <= 1.0, emu.worst
    assert emu.rms * 4 <= oc.RMS_BOUND, emu.rms
    worst_mut = min(oc.check(y, ref.out, ref.M, f16s=True).worst for y in _mutations(brain_conv2).values())
    print(f"emulation: worst err/bound {emu.worst:.3g} (err/M {emu.worst_m:.3g}, rms {emu.rms:.3g}); "
          f"smallest mutation err/bound {worst_mut:.3g}")
    assert worst_mut >= 8.0, worst_mut


def test_checker_on_a_small_magnitude_op(brain_conv2):
    """The same conv scaled down 2^-8 (input, residual, bias, BN mean and offset: outputs and M near 2^-8, most |ref| below
    2^-3, where an F16S lo part is subnormal and the storage floor enters the RMS): the emulation still passes, and the
    dropped hi_x lo_w term - the mutation only the RMS catches - is still flagged."""
    from oracle import ops
    prog, i, state, _, _ = brain_conv2
    op = prog.ops[i]
    s = 2.0 ** -8
    small = copy.copy(prog)
    small.blob = prog.blob.copy()
    for q in range(op.n_stages):
        st = op.stages[q]
        if st.kind == ops.ST_BIAS:
            small.blob[st.p0:st.p0 + op.cout] *= s
        if st.kind == ops.ST_BN:
            small.blob[st.p0:st.p0 + op.cout] *= s
            small.blob[st.p3:st.p3 + op.cout] *= s
    st_small = copy.copy(state)
    st_small.act = {k: (v * s).astype(np.float32) for k, v in state.act.items()}
    ref = ops.run_op(small, i, st_small)
    assert (np.abs(ref.out) < 2.0 ** -3).mean() > 0.9
    emu = oc.check(oc.emulate_conv(small, i, st_small), ref.out, ref.M, f16s=True)
    mut = oc.check(oc.emulate_conv(small, i, st_small, drop_cross=True), ref.out, ref.M, f16s=True)
    print(emu.report("small emulation"), mut.report("small hi_x lo_w dropped"), sep="\n")
    # measured: emulation RMS 1.3e-7 (3.6x under RMS_BOUND - at this scale the INPUT's lo parts are subnormal too, an error
    # of 2^-25 per input element that does not scale with M), the dropped cross term 4.9e-6 (10x over it)
    assert emu.ok and emu.rms * 3 <= oc.RMS_BOUND, emu.rms
    assert not mut.ok and mut.rms >= 8 * oc.RMS_BOUND, mut.rms
