"""Hyena on the CPU tier (the GPU tier is tests/test_gpu_hyena.py):

(1) the float64 restatement's ``causal_conv`` (tests/hyena_reference.py, the direct sum) against a float64 restatement of
    the reference's FFT route, and the properties the reference states for the layer: causality, masked = truncated, zeros
    at masked positions, independent rows, ``|alpha|``, unit norm over exactly ``l`` positions;
(2) the product's host filter table (``program.hyena_filter_tables``) against the restated filter at every tabled row;
(3) a numpy emulation of the kernels' arithmetic sets the per-op bound (a power of two at or above 4 x its own error
    against the restatement, element and RMS error in units of the output's RMS); every mutation lies at least 8 x outside
    it on the input kinds named for it - and the two that are algebraic identities change nothing at all;
(4) the fixtures -> plan -> program, the refusals, the weight names, the loaders;
(5) the new symbols and constants of the C-ABI.
"""
import copy
import ctypes
import re

import numpy as np
import pytest

import attention_reference as ar
import hyena_reference as hr
from conftest import ROOT, load_model_cfg

ALL_OPTIONS = dict(order=2, output_projection=True, filter_normalize=True)
_BOUNDS = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nhyena op: the emulation of the kernels' arithmetic against the restatement (errors in units of the output's rms):")
    for row in _BOUNDS:
        print("  " + row)


def _layer(c=32, seed=3, **params):
    rng = np.random.Generator(np.random.PCG64(seed))
    p = {**hr.params_of({}), **params}
    return hr.random_layer_weights(hr.layer_specs(c, **p), rng), p


# ---- (1) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 2, 166, 665])
def test_direct_sum_against_the_fft_route(l):
    rng = np.random.Generator(np.random.PCG64(l))
    z, h = rng.normal(0, 1, (3, l, 8)), rng.normal(0, 1, (l, 8))
    e, r = ar.errors(hr.causal_conv(z, h), hr.causal_conv_fft(z, h))
    print(f"L {l}: direct sum against the FFT route, max {e:.3g} rms {r:.3g} of the output's rms")
    assert e <= 1e-12


def test_causality():
    w, p = _layer(**ALL_OPTIONS)
    rng = np.random.Generator(np.random.PCG64(1))
    l, t0 = 90, 41
    x = rng.normal(0, 1, (3, l, 32))
    x2 = x.copy()
    x2[:, t0:] = rng.normal(0, 3, (3, l - t0, 32))
    for mask in (None, hr.row_masks(3, l, "n_run")):
        a, b = hr.hyena_block(x, w, mask, **p), hr.hyena_block(x2, w, mask, **p)
        assert np.array_equal(a[:, :t0], b[:, :t0])
        assert np.abs(a[:, t0:] - b[:, t0:]).max() > 0.1


def test_masked_equals_truncated_and_masked_positions_are_zeros():
    rng = np.random.Generator(np.random.PCG64(2))
    l, n = 80, 53
    x = rng.normal(0, 1, (2, l, 32))
    mask = np.zeros((2, l), bool)
    mask[:, :n] = True
    for params in (dict(order=2), dict(order=3, output_projection=True), ALL_OPTIONS):
        w, p = _layer(**params)
        full = hr.hyena_block(x, w, mask, **p)
        short = hr.hyena_block(x[:, :n], w, None, **p)
        assert (full[:, n:] == 0).all()
        if not p["filter_normalize"]:
            e, _ = ar.errors(full[:, :n], short)
            assert e <= 1e-12, e
        else:
            # the filters of the longer call are those of the shorter one times ||h[:n]|| / ||h[:l]|| per order and channel: the
            # operator's output scales by the product over the orders; the output projection and the residual do not scale
            hs, hl = (hr.hyena_filter(w, q, **{**p, "filter_normalize": False}) for q in (n, l))
            ratio = np.prod(np.sqrt((hs * hs).sum(axis=1)) / np.sqrt((hl * hl).sum(axis=1)), axis=0)         # (C)
            g = lambda name: np.asarray(w[name], np.float64)
            unproject = lambda y, xin: np.linalg.solve(g("out_proj/kernel").T, (y - xin - g("out_proj/bias")).reshape(-1, 32).T).T
            e, _ = ar.errors(unproject(full[:, :n], x[:, :n]), unproject(short, x[:, :n]) * ratio[None])
            assert e <= 1e-9, e


def test_rows_are_independent():
    w, p = _layer(**ALL_OPTIONS)
    rng = np.random.Generator(np.random.PCG64(4))
    x = rng.normal(0, 1, (4, 70, 32))
    mask = hr.row_masks(4, 70, "ragged")
    y = hr.hyena_block(x, w, mask, **p)
    x2 = x.copy()
    x2[[0, 1, 3]] = rng.normal(0, 5, (3, 70, 32))
    assert np.array_equal(hr.hyena_block(x2, w, mask, **p)[2], y[2])
    assert np.array_equal(hr.hyena_block(x[2:3], w, mask[2:3], **p)[0], y[2])


def test_negative_alphas_act_as_their_absolute_value_and_normalised_filters_have_unit_norm():
    w, p = _layer(order=2)
    assert (np.asarray(w["hyena/filter/alphas"]) < 0).any()
    w_abs = dict(w)
    w_abs["hyena/filter/alphas"] = np.abs(w["hyena/filter/alphas"])
    assert np.array_equal(hr.hyena_filter(w, 120, **p), hr.hyena_filter(w_abs, 120, **p))
    assert np.abs(hr.hyena_filter(w, 120, mutation="alpha_signed", **p) - hr.hyena_filter(w, 120, **p)).max() > 1e-3
    wz = dict(w)
    last = f"hyena/filter/ffn_0/dense_{p['filter_layers'] - 1}"
    wz[f"{last}/kernel"], wz[f"{last}/bias"] = w[f"{last}/kernel"].copy(), w[f"{last}/bias"].copy()
    wz[f"{last}/kernel"][:, 5] = 0.0                                       # channel 5 of filter 0: all zeros
    wz[f"{last}/bias"][5] = 0.0
    for l in (1, 7, 166):
        h = hr.hyena_filter(wz, l, **{**p, "filter_normalize": True})
        norms = np.sqrt((h * h).sum(axis=1))
        assert (h[0, :, 5] == 0).all() and norms[0, 5] == 0
        keep = np.ones_like(norms, bool)
        keep[0, 5] = False
        assert np.abs(norms[keep] - 1.0).max() <= 1e-12
        longer = hr.hyena_filter(wz, l + 9, **{**p, "filter_normalize": True})[:, :l]
        assert (np.sqrt((longer * longer).sum(axis=1))[keep] < 1.0).all()   # the norm is over exactly l positions


# ---- (2) ----------------------------------------------------------------------------------------------------------------
TABLE_CASES = [dict(filter_activation=a) for a in ("gelu", "sin", "relu", "tanh", "sigmoid", "silu", "swish", "linear", None)] + \
              [dict(filter_layers=n) for n in (1, 2, 3)] + [dict(seq_len=200), dict(seq_len=200, stored=True), dict(order=4, filter_hidden=24)]


@pytest.mark.parametrize("case", TABLE_CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_host_filter_table_against_the_restated_filter(case):
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    case = dict(case)
    stored = case.pop("stored", False)
    w, p = _layer(c=16, seed=9, **case)
    if stored:                                             # a stored encoding wins over the recomputed one: make it differ
        rng = np.random.Generator(np.random.PCG64(5))
        w["hyena/filter/pos_encoding"] = (hr.positional_rows(200) + rng.normal(0, 0.05, (200, 16))).astype(np.float32)
    act = p["filter_activation"]
    layer = P.Hyena("rep/3", 16, p["order"], p["filter_hidden"], p["filter_layers"], None if act in (None, "linear") else act,
                    False, False, p["seq_len"])
    rows = G.hyena_table_rows(layer)
    assert rows == (p["seq_len"] or G.POSITION_ROWS) and G.POSITION_ROWS == hr.TABLE_ROWS
    h, ssq = G.hyena_filter_tables(layer, {f"rep/3/{k}": v for k, v in w.items()})
    want = hr.hyena_filter(w, rows, **p)
    assert h.shape == ssq.shape == (p["order"], rows, 16) and h.dtype == ssq.dtype == np.float32
    # the bound: float32 rounding of the entry (half an ulp), plus 64 ulps of float64 for the two independent evaluations
    tol = np.abs(want) * 2.0 ** -24 + np.abs(want).max() * 2.0 ** -46
    assert (np.abs(h.astype(np.float64) - want) <= tol).all(), float((np.abs(h - want) / np.abs(want).max()).max())
    if stored:
        plain = dict(w)
        del plain["hyena/filter/pos_encoding"]
        assert np.abs(hr.hyena_filter(plain, rows, **p) - want).max() > 1e-4
    for l in (1, 7, 166):
        norm = np.sqrt((want[:, :l] ** 2).sum(axis=1))
        got = np.sqrt(ssq[:, l - 1].astype(np.float64))
        assert (np.abs(got - norm) <= norm * 2.0 ** -22 + 1e-30).all(), (l, float(np.abs(got / norm - 1).max()))


def test_pe_arguments_are_float32_products():
    """What the f32 rounding of the PE arguments alone moves: printed, and held to be small but present."""
    w, p = _layer(seed=9)
    l = 665
    h32 = hr.hyena_filter(w, l, **p)
    pos = np.arange(l, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, 16, 2, dtype=np.float64) * -(np.log(10000.0) / 16))
    exact = np.empty((l, 16))
    exact[:, 0::2], exact[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    w64 = {**w, "hyena/filter/pos_encoding": exact}
    h64 = hr.hyena_filter(w64, l, **{**p, "seq_len": l})
    moved = np.abs(h32 - h64).max() / np.abs(h64).max()
    print(f"f32 PE arguments move filter entries by {moved:.3g} of their maximum at L = {l}")
    assert 1e-9 < moved < 1e-4


# ---- (3) ----------------------------------------------------------------------------------------------------------------
def _op_inputs(l=166, rows=6, c=32):
    out = []
    for name, x in hr.value_inputs(c, rows, l):
        for kind in hr.KINDS:
            out.append((name, kind, x, hr.row_masks(rows, l, kind)))
    return out


@pytest.fixture(scope="module")
def measured():
    """(inputs, reference, bounds) of the all-options layer, computed once and shared."""
    w, p = _layer(**ALL_OPTIONS)
    rows = []
    for name, kind, x, mask in _op_inputs():
        ref = hr.hyena_block(x, w, mask, **p)
        emu = hr.emulate_block(x, w, mask, **p)
        b = ar.bounds_from(emu, ref)
        assert (emu[~mask] == 0).all() if mask is not None else True
        _BOUNDS.append(f"all options  {name:12s} {kind:15s}: max {b['emu_elem']:.3g} (bound {b['elem']:.3g}), rms {b['emu_rms']:.3g} (bound {b['rms']:.3g})")
        rows.append((name, kind, x, mask, ref, b))
    return w, p, rows


def test_the_emulation_sets_the_bound(measured):
    """The per-op bound of the GPU test, measured here: 4 x the emulation's error, rounded up to a power of two.  Also at
    the plain layer, 64 channels at order 3, a second chunk (L 130) and the longest row of the GPU tests (L 665, one input)."""
    worst = max(b["elem"] for *_, b in measured[2])
    for params, c, l, n_in in ((dict(order=2), 32, 166, 4), (dict(order=3, output_projection=True), 64, 166, 1), (ALL_OPTIONS, 32, 130, 1),
                               (dict(order=1), 16, 166, 1), (dict(order=2), 32, 665, 1)):
        w, p = _layer(c=c, **params)
        for name, x in hr.value_inputs(c, 2 if l > 200 else 6, l)[:n_in]:
            for kind in (("ragged",) if l > 200 else ("full", "n_run")):
                mask = hr.row_masks(x.shape[0], l, kind)
                b = ar.bounds_from(hr.emulate_block(x, w, mask, **p), hr.hyena_block(x, w, mask, **p))
                _BOUNDS.append(f"c {c} order {p['order']} L {l} {name:12s} {kind:8s}: max {b['emu_elem']:.3g} (bound {b['elem']:.3g}), rms {b['emu_rms']:.3g} (bound {b['rms']:.3g})")
                worst = max(worst, b["elem"])
    print(f"largest per-op element bound over these inputs: {worst:.3g} of the output's rms")
    # float32 arithmetic: the centring of the "offset rows" (offset 60 x the spread) loses six bits in the layer norm, the two
    # gated convolutions carry that through sums of up to 665 terms - the bound stays below 2^-9 of the output's rms there
    # and below 2^-13 on the inputs without that cancellation
    assert worst <= 2.0 ** -9
    assert max(b["elem"] for name, *_, b in measured[2] if name != "offset rows") <= 2.0 ** -13


@pytest.mark.parametrize("mutation", hr.MUTATIONS)
def test_mutations_land_outside_the_bound(measured, mutation):
    w, p, rows = measured
    seen = set()
    for name, kind, x, mask, ref, b in rows:
        got = hr.hyena_block(x, w, mask, mutation=mutation, **p)
        e, r = ar.errors(got, ref)
        if mutation in hr.INVISIBLE:
            assert np.array_equal(got, ref), (mutation, name, kind)         # an algebraic identity under the exit multiply
            continue
        visible = e >= ar.MUTATION_MARGIN * b["elem"]
        if kind in hr.VISIBLE_ON[mutation]:
            assert visible, f"{mutation} on {name} / {kind}: {e:.3g} against a bound of {b['elem']:.3g}"
            seen.add(kind)
        elif not visible:
            print(f"{mutation}: invisible on {name} / {kind} ({e:.3g})")
    assert seen == set(hr.VISIBLE_ON[mutation])
    assert mutation in hr.INVISIBLE or seen, mutation


def test_every_listed_mutation_is_covered():
    assert set(hr.VISIBLE_ON) == set(hr.MUTATIONS) and all(hr.VISIBLE_ON[m] for m in hr.MUTATIONS if m not in hr.INVISIBLE)
    assert all(not hr.VISIBLE_ON[m] for m in hr.INVISIBLE)


# ---- (4) ----------------------------------------------------------------------------------------------------------------
def _compile(cfg, weights=None):
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    plan = P.build_plan(cfg)
    w = hr.random_weights(cfg) if weights is None else weights
    return plan, G.compile_plan(plan, w), w


def _hyena_at(cfg):
    return [i for i, kind, _ in hr.hyena_layers(cfg) if kind == hr.HYENA]


def _cfg(**over):
    cfg = load_model_cfg("hyena500")
    cfg["representation_learner"]["hidden_layers"][_hyena_at(cfg)[0]]["config"].update(over)
    return cfg


def test_fixture_compiles_to_one_op_with_its_tables():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    cfg = _cfg()
    plan, prog, w = _compile(cfg)
    at = _hyena_at(cfg)[0]
    layer = plan.rep[[i for i, l in enumerate(plan.rep) if isinstance(l, P.Hyena)][0]]
    assert layer == P.Hyena(f"rep/{at}", 32, 2, 32, 2, "gelu", False, False, None)
    assert P.weight_shapes(plan) == hr.weight_specs(cfg)
    ops = [i for i, op in enumerate(prog.ops) if op.kind == L.OP_HYENA]
    assert len(ops) == 1
    op = prog.ops[ops[0]]
    assert (op.cin, op.cout, op.k, op.arg, op.stride, op.dilation) == (32, 32, 2, 0, hr.TABLE_ROWS, 1) and abs(op.f0 - 1e-6) < 1e-12
    assert op.in_buf >= 0 and op.out_buf >= 0 and op.in_buf != op.out_buf and op.in_mask >= 0 and op.out_mask == op.in_mask
    assert [op.stages[s].kind for s in range(op.n_stages)] == [L.ST_BN]                         # the norm rides the op's store
    pool = [o for o in prog.ops if o.kind == L.OP_POOL][0]
    assert pool.in_buf == op.out_buf and pool.in_mask == op.in_mask                              # the mask is kept
    assert any("HYENA" in row and f"order=2 flags=0 table_rows={hr.TABLE_ROWS}" in row for row in prog.describe())
    # the blob: the fold the emulation restates, then the table the restated filter gives, bit for bit / to f32 rounding
    lw = ar.sub_weights(w, f"rep/{at}")
    fw = hr.fold(lw, order=2)
    head = np.concatenate([fw["wp"].ravel(), fw["bp"].ravel()])
    assert np.array_equal(prog.blob[op.w_off:op.w_off + head.size], head)
    table = prog.blob[op.w_off + head.size:op.w_off + head.size + 2 * hr.TABLE_ROWS * 32].reshape(2, hr.TABLE_ROWS, 32)
    want = hr.hyena_filter(lw, hr.TABLE_ROWS, order=2)
    assert (np.abs(table - want) <= np.abs(want) * 2.0 ** -24 + np.abs(want).max() * 2.0 ** -46).all()
    # flags, table rows and the second table
    _, prog2, _ = _compile(_cfg(output_projection=True, filter_normalize=True, seq_len=200, order=3))
    op2 = [o for o in prog2.ops if o.kind == L.OP_HYENA][0]
    assert (op2.k, op2.arg, op2.stride) == (3, L.HYENA_OUT_PROJ | L.HYENA_NORMALIZE, 200)
    # existing models compile as before
    base = _compile(load_model_cfg("baseline500"))[1]
    assert L.OP_HYENA not in [o.kind for o in base.ops]


def test_first_layer_runs_behind_the_identity_conv():
    from jaeger_amd import _lib as L
    cfg = load_model_cfg("hyenafirst500")
    plan, prog, _ = _compile(cfg)
    kinds = [op.kind for op in prog.ops]
    assert kinds == [L.OP_MASK, L.OP_CONV, L.OP_HYENA, L.OP_POOL, L.OP_DENSE]
    mask, conv, op, pool = prog.ops[:4]
    assert conv.in_buf == L.JG_BUF_IDS and conv.k == 1 and conv.in_mask == L.JG_BUF_NONE and conv.n_stages == 0
    assert mask.in_mask == L.JG_BUF_IDS and op.in_mask == mask.out_mask and op.in_buf == conv.out_buf and op.n_stages == 0
    assert pool.in_buf == op.out_buf and pool.in_mask == op.in_mask and plan.pooling == "max" and plan.n_classes == 6


def test_no_mask_behind_cross_frame_attention_and_behind_live_dead_positions():
    from jaeger_amd import _lib as L
    cfg = _cfg()
    at = _hyena_at(cfg)[0]
    cfg["representation_learner"]["hidden_layers"].insert(at, {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)})
    _, prog, _ = _compile(cfg)
    op = [o for o in prog.ops if o.kind == L.OP_HYENA][0]
    assert op.in_mask == L.JG_BUF_NONE and op.out_mask == L.JG_BUF_NONE
    # behind a local_attention with live dead positions: the op is a masked reader, and clears them - an unmasked conv
    # behind it compiles, where it is refused directly behind the local_attention
    import local_attention_reference as lr
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    unmasked = {"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same", use_masking=False)}
    cfg = _cfg()
    layers = cfg["representation_learner"]["hidden_layers"]
    layers.insert(at, {"name": lr.LOCAL, "config": dict(lr.FIXTURE)})
    layers.append(unmasked)
    plan = P.build_plan(cfg)
    G.compile_plan(plan, random_weights(plan))
    del layers[at + 1]
    plan = P.build_plan(cfg)
    with pytest.raises(P.UnsupportedLayer, match="reads masked positions unmasked"):
        G.compile_plan(plan, random_weights(plan))


def test_tail_stages_the_store_cannot_carry_become_ops_behind_it():
    from jaeger_amd import _lib as L
    for norm, lead in (("masked_layernorm", L.ST_LN), ("masked_dyt", L.ST_DYT)):
        cfg = _cfg()
        layers = cfg["representation_learner"]["hidden_layers"]
        layers[-1] = {"name": norm, "config": {}}
        layers.append({"name": "activation", "config": {"activation": "gelu"}})
        _, prog, _ = _compile(cfg)
        kinds = [op.kind for op in prog.ops]
        at = kinds.index(L.OP_HYENA)
        assert prog.ops[at].n_stages == 0 and kinds[at + 1] == L.OP_ELTWISE
        tail = prog.ops[at + 1]
        assert [tail.stages[s].kind for s in range(tail.n_stages)] == [lead, L.ST_ACT] and tail.stages[0].arg == 1
        assert tail.out_mask == prog.ops[at].out_mask and tail.in_buf == tail.out_buf == prog.ops[at].out_buf


@pytest.mark.parametrize("over, word", [
    (dict(dim=64), "dim 64 != 32 incoming channels"),
    (dict(order=0), "order 0"),
    (dict(order=5), "order 5"),
    (dict(filter_layers=0), "filter_layers 0"),
    (dict(filter_activation="elu"), "filter_activation 'elu'"),
    (dict(seq_len=0), "seq_len 0"),
])
def test_plan_refusals_name_the_limit(over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_cfg(**over))


def test_plan_refuses_other_widths_heads_branches_taps_and_entries_the_constructor_would_not_take():
    from jaeger_amd import plan as P
    cfg = _cfg(dim=48)
    for layer in cfg["representation_learner"]["hidden_layers"]:
        if "filters" in layer["config"]:
            layer["config"]["filters"] = 48
    with pytest.raises(P.UnsupportedLayer, match="dim 48 .*16 / 32 / 64"):
        P.build_plan(cfg)
    for act in ("gelu", "sin", "relu", "tanh", "sigmoid", "silu", "swish", "linear", None):
        P.build_plan(_cfg(filter_activation=act))
    P.build_plan(_cfg(order=4, dropout=0.2, kernel_regularizer="l2", kernel_regularizer_w=1e-5, name="h", dtype="float32", trainable=True))
    cfg = load_model_cfg("hyena500")
    cfg["classifier"]["hidden_layers"].insert(0, {"name": hr.HYENA, "config": dict(dim=32)})
    with pytest.raises(P.UnsupportedLayer, match="hyena_block.*head or on a strand branch"):
        P.build_plan(cfg)
    cfg = load_model_cfg("dvf500")
    cfg["representation_learner"]["branch"]["hidden_layers"].insert(1, {"name": hr.HYENA, "config": dict(dim=32)})
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)
    for bad in ({}, dict(order=2), dict(dim=32, num_heads=4), dict(dim=32, pe_dim=16), dict(dim=32, embed_dim=32)):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"][_hyena_at(cfg)[0]]["config"] = dict(bad)
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)
    at = _hyena_at(_cfg())[0]
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"][at + 1]["config"]["return_nmd"] = True
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind hyena_block"):
        P.build_plan(cfg)
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"].insert(at + 1, {"name": "nmd", "config": {}})
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind hyena_block"):
        P.build_plan(cfg)


def test_weight_names_and_shapes():
    from jaeger_amd import plan as P
    cfg = _cfg(order=3, filter_layers=3, filter_hidden=24, output_projection=True)
    at = _hyena_at(cfg)[0]
    shapes = {k: v for k, v in P.weight_shapes(P.build_plan(cfg)).items() if k.startswith(f"rep/{at}/")}
    want = {f"rep/{at}/norm/gamma": (32,), f"rep/{at}/norm/beta": (32,), f"rep/{at}/hyena/filter/alphas": (3, 32),
            f"rep/{at}/hyena/filter/biases": (3, 32), f"rep/{at}/out_proj/kernel": (32, 32), f"rep/{at}/out_proj/bias": (32,)}
    for k in range(4):
        want[f"rep/{at}/hyena/proj_{k}/kernel"] = (32, 32)
    for o in range(3):
        for j, (a, b) in enumerate(((16, 24), (24, 24), (24, 32))):
            want[f"rep/{at}/hyena/filter/ffn_{o}/dense_{j}/kernel"] = (a, b)
            want[f"rep/{at}/hyena/filter/ffn_{o}/dense_{j}/bias"] = (b,)
    assert shapes == want
    one = {k: v for k, v in P.weight_shapes(P.build_plan(_cfg(filter_layers=1, order=1))).items() if "/ffn_" in k}
    assert one == {f"rep/{at}/hyena/filter/ffn_0/dense_0/kernel": (16, 32), f"rep/{at}/hyena/filter/ffn_0/dense_0/bias": (32,)}


def test_stored_positional_encoding_is_optional_and_checked():
    from jaeger_amd import _lib as L
    cfg = _cfg(seq_len=200)
    at = _hyena_at(cfg)[0]
    plan, prog, w = _compile(cfg)
    w2 = dict(w)
    w2[f"rep/{at}/hyena/filter/pos_encoding"] = hr.positional_rows(200).astype(np.float32)
    _, prog2, _ = _compile(cfg, w2)
    op = [o for o in prog.ops if o.kind == L.OP_HYENA][0]
    n = 3 * 32 * 32 + 3 * 32
    a, b = (p_.blob[op.w_off + n:op.w_off + n + 2 * 200 * 32] for p_ in (prog, prog2))
    assert not np.array_equal(a, b) and np.abs(a - b).max() <= np.abs(a).max() * 1e-6      # the stored rows are float32
    w2[f"rep/{at}/hyena/filter/pos_encoding"] = hr.positional_rows(100).astype(np.float32)
    with pytest.raises(ValueError, match="pos_encoding"):
        _compile(cfg, w2)
    # without seq_len the reference stores one row and never reads it: such a variable is ignored
    cfg = _cfg()
    _, prog3, w3 = _compile(cfg)
    w4 = dict(w3)
    w4[f"rep/{at}/hyena/filter/pos_encoding"] = np.zeros((1, 16), np.float32)
    assert np.array_equal(_compile(cfg, w4)[1].blob, prog3.blob)


def test_h5_bundle_and_verify_model_refuse_and_name_the_npz_route(tmp_path):
    from click.testing import CliRunner

    import yaml
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.cli import main
    from jaeger_amd.verify import verify_model
    for name in ("hyena500", "hyenafirst500"):
        cfg = load_model_cfg(name)
        plan = P.build_plan(cfg)
        with pytest.raises(W.AttentionWeightsUnsupported, match=r"hyena_block.*weights\.npz"):
            W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
        with pytest.raises(W.AttentionWeightsUnsupported, match=r"hyena_block.*weights\.npz"):
            W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
        with pytest.raises(P.UnsupportedLayer, match=r"verify-model does not cover hyena_block.*weights\.npz"):
            verify_model(tmp_path / "m_graph", plan)
        w = W.random_weights(plan)
        assert set(w) == set(hr.weight_specs(cfg)) and all(w[k].shape == tuple(v) for k, v in hr.weight_specs(cfg).items())
        W.save_npz(tmp_path / f"{name}.weights.npz", w)
        back = W.load_weights({"weights_npz": tmp_path / f"{name}.weights.npz"}, plan)
        assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    (tmp_path / "g").mkdir()
    (tmp_path / "p.yaml").write_text(yaml.safe_dump({"model": cfg}))
    res = CliRunner().invoke(main, ["verify-model", str(tmp_path / "g"), "--project", str(tmp_path / "p.yaml")])
    assert res.exit_code != 0 and "hyena_block" in res.output and "weights.npz" in res.output


# ---- (5) ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_constants():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    lib = L.load()
    assert lib.jg_hyena_tile() == L.HYENA_TILE == hr.TILE and lib.jg_hyena_chunk() == L.HYENA_CHUNK == hr.CHUNK
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    enum = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", header).group(1))
    assert enum("JG_OP_HYENA") == L.OP_HYENA == L.OP_LENGTHATTN + 1 == 16
    assert lib.jg_sizeof(0) == ctypes.sizeof(L.JgOp)
    kernel_header = (ROOT / "jaeger_amd" / "csrc" / "jg_hyena.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", kernel_header).group(1))
    assert define("JG_HYENA_TILE") == L.HYENA_TILE and define("JG_HYENA_CHUNK") == L.HYENA_CHUNK
    assert define("JG_HYENA_OUT_PROJ") == L.HYENA_OUT_PROJ and define("JG_HYENA_NORMALIZE") == L.HYENA_NORMALIZE
    assert define("JG_HYENA_MAX_ORDER") == L.HYENA_MAX_ORDER == P.HYENA_MAX_ORDER
