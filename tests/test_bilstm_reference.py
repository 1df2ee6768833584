"""CPU tier of the bilstm checks (the GPU tier is tests/test_gpu_bilstm.py):

1. the float64 restatement (tests/bilstm_reference.py) against an independent implementation, ``torch.nn.LSTM(
   bidirectional=True)`` in float64: full rows everywhere; masked rows against torch on the row compressed to its valid
   positions (that is what carrying through masked steps means), then the carried values and the leading / trailing zeros at
   the masked positions;
2. every mutation the issue lists moves the fixture model's logits by more than 100 x the GPU gate of 1e-4 (so the GPU test
   cannot pass with any of them) - but ``masked_step_writes_zeros``, which no masked reader can see: it changes no bit of the
   fixture's outputs, and is held on the ``unmasked_tail`` sibling;
3. the float32 emulation of the kernel's step order stays inside half the gate on the logits of every variant and window
   kind the GPU tier uses;
4. plan, program, weights, refusals, ABI constants.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import attention_reference as ar
import bilstm_reference as br
from conftest import ROOT, load_model_cfg

GATE = 1e-4


# ---- (1) ----------------------------------------------------------------------------------------------------------------
def _torch_bilstm(x, w):
    """torch.nn.LSTM in float64 with Keras' variables: the same gate order i, f, g, o; Keras' single bias in bias_ih, bias_hh = 0."""
    c, u = w["forward/kernel"].shape[0], w["forward/recurrent_kernel"].shape[0]
    net = torch.nn.LSTM(c, u, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in (("forward", ""), ("backward", "_reverse")):
            getattr(net, f"weight_ih_l0{sfx}").copy_(torch.as_tensor(np.asarray(w[f"{d}/kernel"], np.float64).T))
            getattr(net, f"weight_hh_l0{sfx}").copy_(torch.as_tensor(np.asarray(w[f"{d}/recurrent_kernel"], np.float64).T))
            getattr(net, f"bias_ih_l0{sfx}").copy_(torch.as_tensor(np.asarray(w[f"{d}/bias"], np.float64)))
            getattr(net, f"bias_hh_l0{sfx}").zero_()
        return net(torch.as_tensor(np.asarray(x, np.float64)))[0].numpy()


def _layer(c, u, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {}
    for name, shp in br.layer_specs(c, u).items():
        scale = {"kernel": 1.0 / np.sqrt(c), "recurrent_kernel": 1.0 / np.sqrt(u), "bias": 0.1}[name.rsplit("/", 1)[1]]
        w[name] = (rng.normal(0.0, scale, shp)).astype(np.float32)
    return w


@pytest.mark.parametrize("c, u, l", [(16, 16, 1), (32, 32, 41), (64, 16, 17), (48, 64, 30)])
def test_restatement_against_torch_lstm(c, u, l):
    rng = np.random.Generator(np.random.PCG64(l))
    w = _layer(c, u)
    x = rng.normal(0.0, 1.0, (7, l, c))
    want = _torch_bilstm(x, w)
    for mask in (None, np.ones((7, l), bool)):
        assert np.abs(br.bilstm(x, w, mask) - want).max() <= 1e-12
    # masked rows: torch on the row compressed to its valid positions, scattered back; then the carried values
    for kind in br.KINDS[1:]:
        mask = br.hr.row_masks(7, l, kind)
        if l == 1:
            mask[::2] = False
        xm = np.where(mask[..., None], x, 1e6 * rng.normal(0.0, 1.0, x.shape))       # masked values reach nothing
        got = br.bilstm(xm, w, mask)
        assert np.isfinite(got).all()
        at_valid = np.zeros_like(got)
        for r in range(7):
            if mask[r].any():
                at_valid[r, mask[r]] = _torch_bilstm(x[r:r + 1, mask[r]], w)[0]
        assert np.abs(got - at_valid)[mask].max(initial=0.0) <= 1e-12, kind
        assert np.array_equal(got, br.carried_expectation(got, mask)), kind
        for r in range(7):
            valid = np.flatnonzero(mask[r])
            first, last = (valid[0], valid[-1]) if valid.size else (l, -1)
            assert not got[r, :first, :u].any() and not got[r, last + 1:, u:].any(), kind   # leading / trailing zeros
        # ignore_mask: the mask plays no part
        assert np.array_equal(br.bilstm(x, w, mask, ignore_mask=True), br.bilstm(x, w, None))


def test_carried_expectation_on_a_hand_made_row():
    y = np.arange(2 * 6 * 4, dtype=np.float64).reshape(2, 6, 4) + 1.0
    mask = np.array([[0, 1, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0]], bool)
    out = br.carried_expectation(y, mask)
    assert not out[1].any()
    assert np.array_equal(out[0, 0], [0, 0, *y[0, 1, 2:]]) and np.array_equal(out[0, 2], [*y[0, 1, :2], *y[0, 4, 2:]])
    assert np.array_equal(out[0, 3], out[0, 2]) and np.array_equal(out[0, 5], [*y[0, 4, :2], 0, 0])
    assert np.array_equal(out[0, [1, 4]], y[0, [1, 4]])


# ---- (2), (3) -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_refs():
    cfg = br.variant("fixture")
    w = br.random_weights(cfg)
    return cfg, w, {kind: br.forward(cfg, w, br.ids_of(kind, "fixture")) for kind in br.KINDS}


@pytest.mark.parametrize("mutation", br.MUTATIONS)
def test_mutations_move_the_fixture_logits(fixture_refs, mutation):
    """By more than 100 x the gate on the test windows (the largest change over them; every kind on which the mutation can
    show at all must show it far outside float32 rounding, and on the others not one bit changes)."""
    cfg, w, refs = fixture_refs
    name, visible = "fixture", br.VISIBLE_ON[mutation]
    if mutation == "masked_step_writes_zeros":
        for kind in br.KINDS:                      # invisible behind masked readers: not one bit
            got = br.forward(cfg, w, br.ids_of(kind, name), mutation=mutation)
            assert all(np.array_equal(got[k], refs[kind][k]) for k in got), kind
        name, visible = "unmasked_tail", br.VISIBLE_ON["mask_ignored"]
        cfg = br.variant(name)
        w = br.random_weights(cfg)
        refs = {kind: br.forward(cfg, w, br.ids_of(kind, name)) for kind in br.KINDS}
    moved = {}
    for kind in br.KINDS:
        got = br.forward(cfg, w, br.ids_of(kind, name), mutation=mutation)
        moved[kind] = float(np.abs(got["prediction"] - refs[kind]["prediction"]).max())
        print(f"{mutation:30s} {name:14s} {kind:15s} moves the logits by {moved[kind]:.3g}")
        if kind in visible:
            assert moved[kind] > 10 * GATE, (mutation, kind, moved[kind])
        else:
            assert moved[kind] < 1e-12, (mutation, kind, moved[kind])
    assert max(moved.values()) > 100 * GATE, (mutation, moved)


def test_every_listed_mutation_is_covered():
    assert set(br.MUTATIONS) == set(br.VISIBLE_ON) and len(br.MUTATIONS) == 7


@pytest.mark.parametrize("name", br.VARIANTS)
def test_the_emulation_stays_inside_half_the_gate(name, fixture_refs):
    cfg = br.variant(name)
    w = br.random_weights(cfg)
    for kind in br.KINDS:
        ids = br.ids_of(kind, name)
        ref = fixture_refs[2][kind] if name == "fixture" else br.forward(cfg, w, ids)
        emu = br.forward(cfg, w, ids, layer_fn=br.emulate)
        err = float(np.abs(emu["prediction"] - ref["prediction"]).max())
        print(f"{name:14s} {kind:15s} emulation against float64 on the logits: {err:.3g}")
        assert np.isfinite(emu["prediction"]).all() and err <= GATE / 2, (name, kind, err)


def test_stand_in_gains_keep_the_gates_moving():
    """The product's stand-in weights (what a model directory of the tests holds): the layer's outputs neither die nor
    saturate on unit-normal rows of 665 positions."""
    from jaeger_amd import plan as P
    from jaeger_amd.weights import random_weights
    for name in ("fixture", "u64", "stacked"):
        cfg = br.variant(name)
        plan = P.build_plan(cfg)
        w = random_weights(plan)
        for layer in (l for l in plan.rep if isinstance(l, P.BiLstm)):
            x = np.random.Generator(np.random.PCG64(1)).normal(0.0, 1.0, (2, 665, layer.cin))
            y = br.bilstm(x, ar.sub_weights(w, layer.name))
            assert 0.05 < y.std() < 0.6 and (np.abs(y) > 0.99).mean() < 0.01, (name, layer.name, y.std())
            assert y[:, 400:].std() > 0.05


# ---- (4) ----------------------------------------------------------------------------------------------------------------
def _compile(cfg, weights=None):
    from jaeger_amd import plan as P
    from jaeger_amd.program import compile_plan
    from jaeger_amd.weights import random_weights
    plan = P.build_plan(cfg)
    w = random_weights(plan) if weights is None else weights
    return plan, compile_plan(plan, w), w


def _at(cfg):
    return [i for i, kind, _ in br.mixer_layers(cfg) if kind == br.BILSTM]


def _cfg(**over):
    return br.with_bilstm_config(load_model_cfg("bilstm500"), **over)


def test_fixture_compiles_to_one_op():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    cfg = _cfg()
    plan, prog, w = _compile(cfg)
    at = _at(cfg)[0]
    layer = [l for l in plan.rep if isinstance(l, P.BiLstm)][0]
    assert layer == P.BiLstm(f"rep/{at}", 32, 32, False) and layer.channels == 64 and plan.rep_channels == 64
    assert {k: tuple(v) for k, v in P.weight_shapes(plan).items()} == {k: tuple(v) for k, v in br.weight_specs(cfg).items()}
    ops = [o for o in prog.ops if o.kind == L.OP_BILSTM]
    assert len(ops) == 1
    op = ops[0]
    assert (op.cin, op.cout, op.k, op.arg) == (32, 64, 32, 0)
    assert op.in_buf >= 0 and op.out_buf >= 0 and op.in_buf != op.out_buf and op.in_mask >= 0 and op.out_mask == op.in_mask
    assert [op.stages[s].kind for s in range(op.n_stages)] == [L.ST_BN]                         # the norm rides the op's store
    pool = [o for o in prog.ops if o.kind == L.OP_POOL][0]
    assert pool.in_buf == op.out_buf and pool.in_mask == op.in_mask                              # the mask is kept
    assert any("BILSTM" in row and "c=32->64" in row and "units=32 ignore_mask=0" in row for row in prog.describe())
    # the blob: per direction W | R | b, column 64 w + 4 n + g = Keras' column g U + 16 w + n
    lw = ar.sub_weights(w, f"rep/{at}")
    blob = prog.blob[op.w_off:op.w_off + 2 * (32 + 32 + 1) * 128].reshape(2, 65, 128)
    for d, name in enumerate(br.DIRECTIONS):
        full = np.concatenate([lw[f"{name}/kernel"], lw[f"{name}/recurrent_kernel"], lw[f"{name}/bias"][None]])
        for wv in range(2):
            for n in (0, 5, 15):
                for g in range(4):
                    assert np.array_equal(blob[d][:, 64 * wv + 4 * n + g], full[:, g * 32 + 16 * wv + n])
    # ignore_mask: the mask slot is dropped behind the op
    _, prog2, _ = _compile(_cfg(ignore_mask=True, use_cudnn=True, dropout=0.2, recurrent_dropout=0.1, name="b", dtype="float32", trainable=True))
    op2 = [o for o in prog2.ops if o.kind == L.OP_BILSTM][0]
    pool2 = [o for o in prog2.ops if o.kind == L.OP_POOL][0]
    assert op2.arg == L.BILSTM_IGNORE_MASK and op2.in_mask >= 0 and op2.out_mask == L.JG_BUF_NONE and pool2.in_mask == L.JG_BUF_NONE
    # existing models compile as before
    assert L.OP_BILSTM not in [o.kind for o in _compile(load_model_cfg("baseline500"))[1].ops]


def test_variants_compile_first_stacked_and_tails():
    from jaeger_amd import _lib as L
    _, prog, _ = _compile(br.variant("first"))
    assert [op.kind for op in prog.ops] == [L.OP_MASK, L.OP_CONV, L.OP_BILSTM, L.OP_POOL, L.OP_DENSE]
    mask, conv, op = prog.ops[:3]
    assert conv.in_buf == L.JG_BUF_IDS and conv.k == 1 and conv.n_stages == 0 and op.in_mask == mask.out_mask and op.cin == 64
    _, prog, _ = _compile(br.variant("stacked"))
    a, b = [o for o in prog.ops if o.kind == L.OP_BILSTM]
    assert (a.cin, a.k, a.cout, a.n_stages) == (32, 64, 128, 0) and (b.cin, b.k, b.cout) == (128, 16, 32) and b.in_buf == a.out_buf
    assert [b.stages[s].kind for s in range(b.n_stages)] == [L.ST_BN]
    _, prog, _ = _compile(br.variant("behind_cross"))
    op = [o for o in prog.ops if o.kind == L.OP_BILSTM][0]
    assert op.in_mask == L.JG_BUF_NONE and op.out_mask == L.JG_BUF_NONE and op.arg == 0
    _, prog, _ = _compile(br.variant("ln_tail"))
    kinds = [o.kind for o in prog.ops]
    at = kinds.index(L.OP_BILSTM)
    tail = prog.ops[at + 1]
    assert prog.ops[at].n_stages == 0 and tail.kind == L.OP_ELTWISE and tail.cout == 64
    assert [tail.stages[s].kind for s in range(tail.n_stages)] == [L.ST_LN, L.ST_ACT]
    _, prog, _ = _compile(br.variant("then_conv"))
    kinds = [o.kind for o in prog.ops]
    conv = prog.ops[kinds.index(L.OP_BILSTM) + 2]
    assert conv.kind == L.OP_CONV and (conv.cin, conv.cout) == (64, 32)


@pytest.mark.parametrize("over, word", [
    (dict(units=48), r"units 48 .*16 / 32 / 64"),
    (dict(units=128), "units 128"),
    (dict(return_sequences=False), "return_sequences: false .*loses its length axis"),
])
def test_plan_refusals_name_the_limit(over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_cfg(**over))


def test_plan_refuses_other_widths_heads_branches_taps_and_entries_the_constructor_would_not_take():
    from jaeger_amd import plan as P
    for width in (24, 144):
        cfg = _cfg()
        for layer in cfg["representation_learner"]["hidden_layers"]:
            if "filters" in layer["config"]:
                layer["config"]["filters"] = width
        with pytest.raises(P.UnsupportedLayer, match=f"{width} incoming channels .*multiple of 16 up to 128"):
            P.build_plan(cfg)
    cfg = _cfg()
    cfg["classifier"]["hidden_layers"].insert(0, {"name": br.BILSTM, "config": dict(units=32)})
    with pytest.raises(P.UnsupportedLayer, match="masked_bilstm.*head or on a strand branch"):
        P.build_plan(cfg)
    cfg = load_model_cfg("dvf500")
    cfg["representation_learner"]["branch"]["hidden_layers"].insert(1, {"name": br.BILSTM, "config": dict(units=32)})
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)
    for bad in ({}, dict(dropout=0.1), dict(units=32, num_heads=4), dict(units=32, merge_mode="sum"), dict(embed_dim=32, num_heads=4, feed_forward_dim=64)):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"][_at(cfg)[0]]["config"] = dict(bad)
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)
    at = _at(_cfg())[0]
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"][at + 1]["config"]["return_nmd"] = True
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind masked_bilstm"):
        P.build_plan(cfg)
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"].insert(at + 1, {"name": "nmd", "config": {}})
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind masked_bilstm"):
        P.build_plan(cfg)


def test_behind_live_dead_positions_the_masked_layer_runs_and_the_unmasked_one_is_refused():
    import local_attention_reference as lr
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    unmasked = {"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same", use_masking=False)}
    cfg = _cfg()
    at = _at(cfg)[0]
    layers = cfg["representation_learner"]["hidden_layers"]
    layers.insert(at, {"name": lr.LOCAL, "config": dict(lr.FIXTURE)})
    layers.append(unmasked)                        # behind the masked bilstm no dead position is live any more
    plan = P.build_plan(cfg)
    G.compile_plan(plan, random_weights(plan))
    layers[at + 1]["config"]["ignore_mask"] = True
    del layers[-1]
    plan = P.build_plan(cfg)
    with pytest.raises(P.UnsupportedLayer, match="masked_bilstm with ignore_mask.*reads masked positions unmasked"):
        G.compile_plan(plan, random_weights(plan))


def test_weight_names_and_shapes():
    from jaeger_amd import plan as P
    cfg = br.variant("stacked")
    a, b = _at(cfg)
    shapes = {k: v for k, v in P.weight_shapes(P.build_plan(cfg)).items() if k.startswith((f"rep/{a}/", f"rep/{b}/"))}
    want = {}
    for at, c, u in ((a, 32, 64), (b, 128, 16)):
        for d in ("forward", "backward"):
            want.update({f"rep/{at}/{d}/kernel": (c, 4 * u), f"rep/{at}/{d}/recurrent_kernel": (u, 4 * u), f"rep/{at}/{d}/bias": (4 * u,)})
    assert shapes == want


def test_h5_bundle_and_verify_model_refuse_and_name_the_npz_route(tmp_path):
    from click.testing import CliRunner

    import yaml
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.cli import main
    from jaeger_amd.verify import verify_model
    cfg = load_model_cfg("bilstm500")
    plan = P.build_plan(cfg)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"masked_bilstm.*weights\.npz"):
        W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"masked_bilstm.*weights\.npz"):
        W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
    with pytest.raises(P.UnsupportedLayer, match=r"verify-model does not cover masked_bilstm.*weights\.npz"):
        verify_model(tmp_path / "m_graph", plan)
    w = W.random_weights(plan)
    assert set(w) == set(br.weight_specs(cfg)) and all(w[k].shape == tuple(v) for k, v in br.weight_specs(cfg).items())
    W.save_npz(tmp_path / "bilstm500.weights.npz", w)
    back = W.load_weights({"weights_npz": tmp_path / "bilstm500.weights.npz"}, plan)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    (tmp_path / "g").mkdir()
    (tmp_path / "p.yaml").write_text(yaml.safe_dump({"model": cfg}))
    res = CliRunner().invoke(main, ["verify-model", str(tmp_path / "g"), "--project", str(tmp_path / "p.yaml")])
    assert res.exit_code != 0 and "masked_bilstm" in res.output and "weights.npz" in res.output


def test_abi_symbols_and_constants():
    from jaeger_amd import _lib as L
    lib = L.load()
    assert lib.jg_bilstm_rows() == L.BILSTM_ROWS == br.ROWS and lib.jg_bilstm_steps() == L.BILSTM_STEPS == br.STEPS
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    enum = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", header).group(1))
    assert enum("JG_OP_BILSTM") == L.OP_BILSTM == L.OP_HYENA + 1 == 17
    assert lib.jg_sizeof(0) == ctypes.sizeof(L.JgOp)
    kernel_header = (ROOT / "jaeger_amd" / "csrc" / "jg_bilstm.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", kernel_header).group(1))
    assert define("JG_BILSTM_ROWS") == L.BILSTM_ROWS and define("JG_BILSTM_STEPS") == L.BILSTM_STEPS
    assert define("JG_BILSTM_IGNORE_MASK") == L.BILSTM_IGNORE_MASK
