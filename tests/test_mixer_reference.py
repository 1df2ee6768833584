"""The CPU tier of the row-mixer pair checks (the GPU tier is tests/test_gpu_mixer_pairs.py; the reference side
tests/mixer_reference.py).  No GPU, no built library: the composed float64 forward against the six modules' own forwards, the
7 x 7 table of ordered pairs through ``build_plan`` / ``compile_plan`` against the mask rule per layer, and the proof that a
broken hand-over between two mixers is visible at the model's outputs.

* the unified forward adds no semantics: on every variant of the six reference modules it equals that module's own
  ``forward`` bit for bit, with that module's own weights (every variant on two window kinds of the module, one without and
  one with masked positions: the six full cross products are 400 forwards of up to a second each);
* all 49 ordered pairs: 46 compile, 3 are refused with the reason; per compiled program the mask slot every layer reads and
  the op that wrote it follow :data:`mixer_reference.MASK_BEHIND` - asserted from that table and from
  :func:`mixer_reference.layer_ops`, not from what the compiler does;
* the hand-over mutations (``stale``, ``dropped``) move the logits by at least 8 x the project's gate of 1e-4 - or, for a second
  layer of ``cross_frame_attention``, by exactly nothing: that layer reads no mask and leaves none, so that hand-over is
  held by the per-op mask assertions of the pair table alone.  Measured minima over the compiled pairs: 5.7e-3 under
  ``stale`` and 1.8e-2 under ``dropped``, both at msconv -> bilstm (the table prints at the end of the module);
* behind a local_attention the dead positions are never read: 1e3 or 0 there, every output is the same bit for bit;
* the input conditions of all this, asserted so that none of it can go vacuous.
"""
import functools

import numpy as np
import pytest

import attention_reference as ar
import axial_attention_reference as xr
import bilstm_reference as br
import hyena_reference as hr
import local_attention_reference as lr
import mixer_reference as mx
import multiscale_reference as mr
import test_gpu_axialattn as gpu_axial
import test_gpu_frameattn as gpu_frame
import test_gpu_hyena as gpu_hyena
import test_gpu_localattn as gpu_local

GATE = 1e-4
MARGIN = ar.MUTATION_MARGIN          # the project's convention: a mutation shows at 8 x the bound (tests/op_cases.py)
PAIRS = [(a, b) for a in mx.KINDS for b in mx.KINDS]
COMPILED = [p for p in PAIRS if p not in mx.REFUSED]
_MOVED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _MOVED:
        print("\nhand-over mutations on long_n: largest change of a logit (gate 1e-4)")
        for (a, b), row in sorted(_MOVED.items()):
            print(f"  {a:8s} -> {b:8s}  " + "  ".join(f"{h} {v:.2e}" for h, v in sorted(row.items())))
        for h in mx.HANDOVERS:
            rows = [(v[h], p) for p, v in _MOVED.items() if h in v and p[1] != "cross" and v[h] > 0]
            if rows:
                print(f"  smallest required change under {h}: {min(rows)[0]:.2e} at {' -> '.join(min(rows)[1])}")


@functools.lru_cache(maxsize=None)
def _pair(a, b):
    cfg = mx.pair_cfg(a, b)
    return cfg, mx.random_weights(cfg)


@functools.lru_cache(maxsize=None)
def _ids(kind):
    ids = mx.ids_of(kind)
    ids.setflags(write=False)
    return ids


# ---- a. the unified forward adds no semantics of its own ----------------------------------------------------------------
def _frame_ids(kind, name):
    from oracle import encoder as oenc
    return ar.window_ids(oenc.frame_length(gpu_frame.FSIZE), kind, 2, 17)


def _local_ids(kind, name):
    cfg = gpu_local.variant(name)
    half = [int(a["window_size"]) // 2 for _, k, a in lr.attention_layers(cfg) if k == lr.LOCAL][0]
    return gpu_local.ids_of(kind, half, n_win=2)


#: module -> (its variants, variant(name), its weights, its forward, ids(kind, name), the two window kinds)
MODULES = {
    "frame": (gpu_frame.VARIANTS, gpu_frame.variant, ar.random_weights, ar.forward, _frame_ids, ("full", "ragged")),
    "local": (gpu_local.VARIANTS, gpu_local.variant, lr.random_weights, lr.forward, _local_ids, ("full", "long_n")),
    "axial": (gpu_axial.VARIANTS, gpu_axial.variant, xr.random_weights, xr.forward, lambda k, n: gpu_axial.ids_of(k, n_win=2), ("full", "empty_fwd")),
    "hyena": (gpu_hyena.VARIANTS, gpu_hyena.variant, hr.random_weights, hr.forward, lambda k, n: gpu_hyena.ids_of(k, n, n_win=2), ("full", "n_run")),
    "bilstm": (br.VARIANTS, br.variant, br.random_weights, br.forward, lambda k, n: br.ids_of(k, n, n_win=2), ("full", "many_runs")),
    "multiscale": (mr.VARIANTS, mr.variant, mr.random_weights, mr.forward, lambda k, n: mr.ids_of(k, n_win=2), ("full", "islands")),
}


@pytest.mark.parametrize("module, name", [(m, n) for m, row in MODULES.items() for n in row[0]])
def test_unified_forward_equals_the_modules_own(module, name):
    _, variant, weights_of, forward, ids_of, kinds = MODULES[module]
    cfg = variant(name)
    weights = weights_of(cfg)
    masked = 0
    for kind in kinds:
        ids = ids_of(kind, name)
        masked += int((ids == 0).sum())
        want = forward(cfg, weights, ids)
        got = mx.forward(cfg, weights, ids)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{module} / {name} / {kind}: {k}")
    assert masked > 0


def test_weight_specs_are_each_modules_own():
    """On a model one module alone understands, the unified specs are that module's."""
    for module, (variants, variant, _, _, _, _) in MODULES.items():
        specs_of = {"frame": ar.weight_specs, "local": lr.weight_specs, "axial": xr.weight_specs, "hyena": hr.weight_specs,
                    "bilstm": br.weight_specs, "multiscale": mr.weight_specs}[module]
        for name in variants:
            cfg = variant(name)
            assert mx.weight_specs(cfg) == specs_of(cfg), (module, name)


def test_random_weights_follow_each_layers_rules():
    cfg = mx.chain_cfg("masked_first")
    w = mx.random_weights(cfg)
    assert {k: v.shape for k, v in w.items()} == mx.weight_specs(cfg) and all(v.dtype == np.float32 for v in w.values())
    by_kind = {mx.SHORT[kind]: f"rep/{i}" for i, kind, _ in mx.mixer_layers(cfg)}
    assert set(by_kind) == set(mx.KINDS)
    bias = w[by_kind["bilstm"] + "/forward/bias"]
    u = bias.shape[0] // 4
    assert bias[u:2 * u].mean() > 0.8 and abs(bias[:u].mean()) < 0.2                       # the forget gate's plus one
    rec = w[by_kind["bilstm"] + "/forward/recurrent_kernel"]
    assert abs(rec.var() * u - 1.0) < 0.25                                                  # orthogonal scale: variance 1 / U
    last = w[by_kind["hyena"] + "/hyena/filter/ffn_0/dense_1/kernel"]
    first = w[by_kind["hyena"] + "/hyena/filter/ffn_0/dense_0/kernel"]
    glorot = np.sqrt(6.0 / last.shape[0])
    assert np.abs(last).max() <= glorot * hr.FILTER_GAIN and np.abs(first).max() > 4 * np.abs(last).max()
    assert (w[by_kind["hyena"] + "/hyena/filter/alphas"] < 0).any()
    assert mx.random_weights(cfg, 5)["classifier/1/kernel"].tobytes() != w["classifier/1/kernel"].tobytes()


# ---- b. the pair table ---------------------------------------------------------------------------------------------------
def _compile(cfg, weights):
    from jaeger_amd import plan as P
    from jaeger_amd.program import compile_plan
    return compile_plan(P.build_plan(cfg), weights)


def _mask_source(prog, i, slot):
    """The op that wrote mask slot ``slot`` as op ``i`` sees it (None for no slot)."""
    from jaeger_amd import _lib as L
    if slot == L.JG_BUF_NONE:
        return None
    assert slot >= 0, (i, slot)
    for j in range(i - 1, -1, -1):
        o = prog.ops[j]
        if o.out_mask == slot and o.kind in (L.OP_MASK, L.OP_MSMASK, L.OP_EMBED):
            return j
    raise AssertionError(f"op {i}: nothing wrote mask slot {slot}")


def check_program(cfg, prog):
    """The hand-over of every mixer layer of ``prog`` against the rule table: which mask slot each layer reads, which op wrote
    it, which activation each op reads - and the slot bookkeeping around them."""
    from jaeger_amd import _lib as L
    layers = mx.layer_ops(cfg, prog)
    ops = prog.ops
    mixer_kinds = (L.OP_FRAMEATTN, L.OP_LOCALATTN, L.OP_LENGTHATTN, L.OP_HYENA, L.OP_BILSTM, L.OP_MSCONV)
    for i, op in enumerate(ops):
        slots = [op.in_buf, op.out_buf, op.in_mask, op.out_mask] + [op.stages[s].arg for s in range(op.n_stages) if op.stages[s].kind == L.ST_ADD]
        assert max(slots) < L.JG_MAX_BUFS, (i, slots)
        if op.kind in mixer_kinds:
            assert op.in_buf != op.out_buf and op.in_buf >= 0 and op.out_buf >= 0, (i, "in place")
        if op.kind == L.OP_MSCONV and op.in_mask != L.JG_BUF_NONE:
            m = ops[i - 1]
            assert m.kind == L.OP_MSMASK and (m.w_off, m.in_mask, m.out_mask) == (op.w_off, op.in_mask, op.out_mask), i
            assert m.out_mask != m.in_mask and m.out_mask >= 0
        if op.kind == L.OP_MSMASK:
            assert ops[i + 1].kind == L.OP_MSCONV
    # the walk: (mask slot, the op that wrote it) as the rule table hands them from layer to layer
    first = layers[0][3][0]
    act = mx.producer(prog, next(i for i in layers[0][3] if ops[i].kind != L.OP_MSMASK))
    slot = ops[act].out_mask                     # the mask of the conv in front: what arrives at the first mixer
    assert ops[act].kind == L.OP_CONV and slot >= 0, "no mask slot arrives at the first mixer"
    source = _mask_source(prog, first, slot)
    assert ops[source].kind == L.OP_MASK
    for short, _, a, idxs in layers:
        masked = slot != L.JG_BUF_NONE
        for n, i in enumerate(idxs):
            op = ops[i]
            where = f"{short} op {i}"
            # which of its ops read the layer's incoming mask
            if op.kind == L.OP_FRAMEATTN:
                want = L.JG_BUF_NONE
            elif op.kind == L.OP_LENGTHATTN:
                want = slot if n == 0 else L.JG_BUF_NONE                 # (an axial layer's block 0 alone)
            elif op.kind == L.OP_ELTWISE:
                want = L.JG_BUF_NONE                                       # (it reads out_mask, below)
            else:
                want = slot
            assert op.in_mask == want, (where, "in_mask", op.in_mask, want)
            if want != L.JG_BUF_NONE:
                assert _mask_source(prog, i, want) == source, (where, "mask slot rewritten", _mask_source(prog, i, want), source)
            if op.kind == L.OP_MSMASK:
                continue
            # the activation chain: every op reads what the op in front of it wrote, into another slot
            assert mx.producer(prog, i) == act, (where, "in_buf", mx.producer(prog, i), act)
            if op.kind == L.OP_ELTWISE:
                assert op.in_buf == op.out_buf and ops[act].out_buf == op.in_buf
                adds = [op.stages[s].arg for s in range(op.n_stages) if op.stages[s].kind == L.ST_ADD]
                block_in = mx.producer(prog, idxs[n - 2])
                assert len(adds) == 1 and mx.producer(prog, i, adds[0]) == block_in, (where, "the block's input was overwritten")
                assert op.out_mask == slot and (not masked or _mask_source(prog, i, slot) == source), where
            act = i
        # the mask behind the layer
        rule = mx.MASK_BEHIND[short]
        if short == "bilstm" and a.get("ignore_mask"):
            rule = "none"
        last = ops[idxs[-1]]
        if rule == "none" or not masked:
            slot, source = L.JG_BUF_NONE, None
        elif rule == "own":
            m = idxs[0]
            assert ops[m].kind == L.OP_MSMASK
            slot, source = ops[m].out_mask, m
        assert last.out_mask == slot, (short, "out_mask", last.out_mask, slot)
    # behind the last mixer: everything up to the pool reads that mask, as that op wrote it
    pool = next(i for i, op in enumerate(ops) if op.kind == L.OP_POOL)
    for i in range(layers[-1][3][-1] + 1, pool + 1):
        op = ops[i]
        got = op.in_mask if op.kind == L.OP_POOL else op.out_mask
        assert got == slot, (i, "the mask behind the last mixer", got, slot)
        if slot != L.JG_BUF_NONE:
            assert _mask_source(prog, i, slot) == source, (i, "mask slot rewritten")
        assert mx.producer(prog, i) == act
        act = i if op.out_buf >= 0 else act
    return layers


@pytest.mark.parametrize("a, b", PAIRS)
def test_pair_table(a, b):
    from jaeger_amd import _lib as L
    from jaeger_amd.plan import UnsupportedLayer
    cfg, weights = _pair(a, b)
    if (a, b) in mx.REFUSED:
        phrase = {"cross": "cross_frame_attention", "encoder": "transformer_encoder", "axial": "axial_attention"}[b]
        with pytest.raises(UnsupportedLayer, match=r"behind .* \(local_attention\)") as exc:
            _compile(cfg, weights)
        assert f": {phrase} (" in str(exc.value) and "reads masked positions unmasked" in str(exc.value)
        return
    prog = _compile(cfg, weights)
    layers = check_program(cfg, prog)
    assert [row[0] for row in layers] == [a, b]
    # the issue's statement of the rule, on the second layer's first op
    first, second = prog.ops[layers[0][3][0]], prog.ops[layers[1][3][0]]
    if b == "cross" or mx.MASK_BEHIND[a] == "none":          # (a cross_frame_attention reads no mask, whatever arrives)
        want = L.JG_BUF_NONE
    elif mx.MASK_BEHIND[a] == "kept":
        want = first.in_mask
        assert want >= 0
    else:
        assert first.kind == L.OP_MSMASK
        want = first.out_mask
    assert second.in_mask == want


def test_exactly_three_pairs_are_refused():
    from jaeger_amd.plan import UnsupportedLayer
    refused = []
    for a, b in PAIRS:
        try:
            _compile(*_pair(a, b))
        except UnsupportedLayer:
            refused.append((a, b))
    assert tuple(refused) == mx.REFUSED and len(PAIRS) - len(refused) == 46


@pytest.mark.parametrize("a, b", mx.WIDE)
def test_wide_handover_programs(a, b):
    """A slot that holds rows of two widths in one forward: the same walk."""
    from jaeger_amd import _lib as L
    cfg = mx.wide_cfg(a, b)
    prog = _compile(cfg, mx.random_weights(cfg))
    layers = check_program(cfg, prog)
    widths = [(prog.ops[idxs[0]].cin, prog.ops[idxs[-1]].cout) for _, _, _, idxs in layers]
    assert widths == ([(32, 128), (128, 32)] if a == "bilstm128" else [(32, 64), (64, 64)])
    if a == "bilstm128":                    # the 32-wide rows go back into a slot that held 32-wide rows in front of the 128-wide ones
        by_slot = {}
        for op in prog.ops:
            if op.out_buf >= 0 and op.kind != L.OP_ELTWISE:
                by_slot.setdefault(op.out_buf, set()).add(op.cout)
        assert any(len(v) > 1 for v in by_slot.values()), by_slot


@pytest.mark.parametrize("name", mx.CHAINS)
def test_chain_programs(name):
    from jaeger_amd import _lib as L
    cfg = mx.chain_cfg(name)
    prog = _compile(cfg, mx.random_weights(cfg))
    layers = check_program(cfg, prog)
    assert tuple(row[0] for row in layers) == mx.CHAINS[name]
    kinds = {op.kind for op in prog.ops}
    assert {L.OP_FRAMEATTN, L.OP_LOCALATTN, L.OP_LENGTHATTN, L.OP_HYENA, L.OP_BILSTM, L.OP_MSCONV} <= kinds
    assert (L.OP_MSMASK in kinds) == (name == "masked_first")
    masked = [prog.ops[idxs[0]].in_mask != L.JG_BUF_NONE for _, _, _, idxs in layers]
    assert masked == ([True] * 6 + [False] if name == "masked_first" else [False] * 7)      # (a cross_frame_attention reads none)


# ---- c. the hand-over is visible ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("a, b", COMPILED)
def test_a_broken_handover_moves_the_logits(a, b):
    """``stale`` must show behind the first layers that change or drop the mask, ``dropped`` behind those that keep or write
    one.  A second layer of cross_frame_attention reads no mask and leaves none: the mutation cannot reach the outputs (the
    change is exactly zero), and that hand-over is held by the per-op mask assertions of test_pair_table alone."""
    cfg, weights = _pair(a, b)
    ids = _ids("long_n")
    ref = mx.forward(cfg, weights, ids)
    required = {"stale": a in ("cross", "encoder", "msconv"), "dropped": a in ("local", "axial", "hyena", "bilstm", "msconv")}
    assert any(required.values())
    row = _MOVED.setdefault((a, b), {})
    for handover in mx.HANDOVERS:
        with np.errstate(over="ignore"):          # (a bilstm that reads a local layer's dead positions unmasked saturates)
            got = mx.forward(cfg, weights, ids, handover=handover)
        moved = float(np.abs(got["prediction"] - ref["prediction"]).max())
        row[handover] = moved
        print(f"{a} -> {b} {handover}: {moved:.3e}")
        if b == "cross":
            for k in ref:
                np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{a} -> cross, {handover}: {k}")
        elif required[handover]:
            assert moved >= MARGIN * GATE, (a, b, handover, moved)
        else:                                       # the mutation IS the rule here: nothing changes
            assert moved == 0.0, (a, b, handover, moved)


# ---- d. dead positions are never read -------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ["local", "hyena", "bilstm", "msconv"])
def test_dead_positions_behind_a_local_layer_are_never_read(b):
    cfg, weights = _pair("local", b)
    for kind in ("long_n", "empty_row"):
        info = []
        loud = mx.forward(cfg, weights, _ids(kind), dead_fill=1e3, info=info)
        quiet = mx.forward(cfg, weights, _ids(kind), dead_fill=0.0)
        assert int(info[0]["dead"].sum()) > 0
        for k in loud:
            np.testing.assert_array_equal(loud[k], quiet[k], err_msg=f"local -> {b} / {kind}: {k}")


# ---- e. the input conditions ----------------------------------------------------------------------------------------------
def test_input_conditions():
    assert not (_ids("full") == 0).any()
    assert (_ids("empty_row") == 0).all(axis=2).sum() >= 2 and (_ids("empty_row") != 0).any(axis=2).sum() >= 12
    for kind in mx.WINDOW_KINDS:
        assert _ids(kind).shape == (3, 6, 165)
    # every local layer leaves dead positions with valid ones on both sides in some row; every masked msconv returns a mask
    # that differs from the one it read
    seen = {"local": 0, "msconv": 0}
    for a, b in (("local", "local"), ("msconv", "local"), ("local", "msconv"), ("msconv", "msconv"), ("axial", "local"), ("hyena", "msconv")):
        cfg, weights = _pair(a, b)
        info = []
        mx.forward(cfg, weights, _ids("long_n"), info=info)
        assert [row["kind"] for row in info] == [a, b]
        for row in info:
            m = row["mask_in"]
            assert m is not None and m.shape == (3, 6, 159) and (~m).sum() > 0, "no invalid position reached the mixer"
            if row["kind"] == "local":
                dead = row["dead"].reshape(-1, 159)
                m2 = m.reshape(-1, 159)
                before, behind = m2.cumsum(axis=1) > 0, m2[:, ::-1].cumsum(axis=1)[:, ::-1] > 0
                assert (dead & before & behind).any(), f"{a} -> {b}: no dead position with valid ones on both sides"
                assert not (dead & m2).any()
                seen["local"] += 1
            if row["kind"] == "msconv":
                assert (row["mask_out"] != m).sum() > 0 and not (~row["mask_out"] & m).any()      # (it grows, and only grows)
                seen["msconv"] += 1
    assert seen == {"local": 5, "msconv": 5}
    info = []
    mx.forward(*_pair("local", "local"), _ids("long_n"), info=info)
    assert [int(row["dead"].sum()) for row in info] == [36, 36]
    info = []
    mx.forward(*_pair("msconv", "local"), _ids("long_n"), info=info)
    assert int(info[1]["dead"].sum()) == 18 and int((info[0]["mask_out"] != info[0]["mask_in"]).sum()) == 18
    # grow = 0 is the trap: the convs in front heal the run and nothing invalid reaches the mixers
    info = []
    mx.forward(*_pair("hyena", "hyena"), hr.window_ids(165, "n_run", n_win=3, seed=17, grow=0), info=info)
    assert (~info[0]["mask_in"]).sum() == 0


def test_producer_and_mask_writer_go_by_slots_alone():
    """A multi-scale conv behind a bilstm, a bilstm behind a multi-scale conv: the private copies these replace knew neither."""
    from jaeger_amd import _lib as L
    cfg, weights = _pair("bilstm", "msconv")
    prog = _compile(cfg, weights)
    (_, _, _, (lstm,)), (_, _, _, (msmask, msconv)) = mx.layer_ops(cfg, prog)
    assert mx.producer(prog, msconv) == lstm and prog.ops[mx.mask_writer(prog, msconv)].kind == L.OP_MASK
    assert mx.mask_writer(prog, msmask) == mx.mask_writer(prog, lstm)
    cfg, weights = _pair("msconv", "bilstm")
    prog = _compile(cfg, weights)
    (_, _, _, (msmask, msconv)), (_, _, _, (lstm,)) = mx.layer_ops(cfg, prog)
    assert mx.producer(prog, lstm) == msconv and mx.mask_writer(prog, lstm) == msmask
    cfg, weights = _pair("cross", "hyena")
    prog = _compile(cfg, weights)
    assert mx.mask_writer(prog, mx.layer_ops(cfg, prog)[1][3][0]) is None
    with pytest.raises(AssertionError):
        mx.producer(prog, 0)                  # the first op reads the id tensor: no activation slot
