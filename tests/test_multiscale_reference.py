"""The multi-scale conv on the CPU: (1) the float64 restatement of MultiScaleConv1D (tests/multiscale_reference.py) against an
independent convolution - ``torch.nn.functional.conv1d`` with explicit TF-SAME padding; (2) every listed mutation changes the
restated op and moves the logits of the model named for it by more than the 1e-4 gate on the window kinds ``VISIBLE_ON``
lists, the mask mutations change the layer's mask on ``islands``, and on ``islands`` the fixture's output mask differs from
every single branch's - so the window kinds cannot go blind; (3) plan and program: defaults, channel count, the blob's
descriptor, the op fields, the mask op in front of the mixer, what compiles behind the layer; (4) every refusal with its
wording, and the generic fall-through; (5) weights; (6) the numpy emulation of the kernel's f32 arithmetic stays within 1e-5 of
the restatement.  The GPU tier is tests/test_gpu_multiscale.py.
"""
import copy
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_reference as ar
import multiscale_reference as mr
from conftest import load_model_cfg

ROOT = Path(__file__).resolve().parent.parent
GATE = 1e-4
N_WIN = 2            # windows of the model forwards here (the GPU tier runs five)


# ---- (1) ----------------------------------------------------------------------------------------------------------------
def _kd_of_the_variants():
    out = set()
    for name in mr.VARIANTS:
        for _, kind, a in mr.mixer_layers(mr.variant(name)):
            if kind == mr.MSCONV:
                out |= {(b["kernel_size"], b["dilation_rate"]) for b in mr.branch_params(a)}
    return sorted(out)


def _independent_conv(x, kernel, bias, k, d):
    """(R, L, C) -> (R, L, F): conv1d on (R, C, L) behind explicit TF-SAME padding: (k - 1) d // 2 zeros on the left, the rest
    on the right."""
    total = (k - 1) * d
    xp = F.pad(torch.as_tensor(x).permute(0, 2, 1), (total // 2, total - total // 2))
    y = F.conv1d(xp, torch.as_tensor(kernel).permute(2, 1, 0).contiguous(), torch.as_tensor(bias), dilation=d)
    return y.permute(0, 2, 1).numpy()


def test_restatement_against_an_independent_conv():
    kd = _kd_of_the_variants()
    assert {(3, 1), (5, 1), (3, 3), (4, 1), (2, 5), (15, 1), (5, 16), (2, 1), (1, 1)} <= set(kd), kd
    rng = np.random.Generator(np.random.PCG64(3))
    for k, d in kd:
        c, fl = 16, 8
        lw = {"branch0/kernel": rng.normal(0, 0.3, (k, c, fl)), "branch0/bias": rng.normal(0, 0.1, fl),
              "branch1/kernel": rng.normal(0, 0.3, (3, c, fl)), "branch1/bias": rng.normal(0, 0.1, fl)}
        p = dict(merge="concat", branches=[dict(filters=fl, kernel_size=k, dilation_rate=d, activation=None, use_bias=True, use_masking=True, mask_mode="any"),
                                           dict(filters=fl, kernel_size=3, dilation_rate=1, activation=None, use_bias=True, use_masking=True, mask_mode="any")])
        for l in sorted({1, 2, max(k - 1, 1), 37, 166}):
            x = rng.normal(0, 1, (3, l, c))
            mask = rng.random((3, l)) > 0.3
            y, om = mr.rows_op(x, mask, lw, p)
            xm = x * mask[..., None]
            want = np.concatenate([_independent_conv(xm, lw["branch0/kernel"], lw["branch0/bias"], k, d),
                                   _independent_conv(xm, lw["branch1/kernel"], lw["branch1/bias"], 3, 1)], axis=-1)
            assert np.abs(y - want).max() <= 1e-12, (k, d, l, np.abs(y - want).max())
            # the mask, by the definition: the branch's rule on the count of valid taps at t + j d - (k - 1) d // 2 inside the row
            pl = (k - 1) * d // 2
            cnt = np.array([[sum(0 <= t + j * d - pl < l and mask[r, t + j * d - pl] for j in range(k)) for t in range(l)] for r in range(3)])
            cnt3 = np.array([[sum(0 <= t + j - 1 < l and mask[r, t + j - 1] for j in range(3)) for t in range(l)] for r in range(3)])
            assert np.array_equal(om, (cnt > 0) & (cnt3 > 0)), (k, d, l)
            p2 = copy.deepcopy(p)
            p2["branches"][0]["mask_mode"], p2["branches"][1]["mask_mode"] = "majority", "strict"
            assert np.array_equal(mr.rows_op(x, mask, lw, p2)[1], (cnt >= (k + 1) // 2) & (cnt3 == 3)), (k, d, l)
            # add: the plain sum; no mask arrives: none leaves
            p3 = dict(p, merge="add")
            assert np.abs(mr.rows_op(x, mask, lw, p3)[0] - (want[..., :fl] + want[..., fl:])).max() <= 1e-12
            assert mr.rows_op(x, None, lw, p)[1] is None
    # branches that do not mask: the values at masked positions are read, no mask leaves
    p4 = copy.deepcopy(p)
    for b in p4["branches"]:
        b["use_masking"] = False
    y, om = mr.rows_op(x, mask, lw, p4)
    assert om is None and np.abs(y[..., :fl] - _independent_conv(x, lw["branch0/kernel"], lw["branch0/bias"], k, d)).max() <= 1e-12


# ---- (2) ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    out = {}
    for name in sorted(set(mr.MODEL_OF.values())):
        cfg = mr.variant(name)
        w = mr.random_weights(cfg)
        out[name] = (cfg, w, {kind: mr.forward(cfg, w, mr.ids_of(kind, N_WIN))["prediction"] for kind in mr.KINDS})
    return out


def _layer_inputs(name, kind):
    """(x, mask, lw, params) of the model's multi-scale layer on the rows of ``kind``: directly behind the embedding."""
    cfg = mr.variant(name)
    w = mr.random_weights(cfg)
    (at, k_, a), = [m for m in mr.mixer_layers(cfg) if m[1] == mr.MSCONV]
    assert at == 0
    ids = mr.ids_of(kind).reshape(-1, mr.ids_of(kind).shape[2])
    return w["embedding/embeddings"][ids].astype(np.float64), ids != 0, ar.sub_weights(w, "rep/0"), mr.params_of(a)


@pytest.mark.parametrize("mutation", mr.MUTATIONS)
def test_every_mutation_changes_the_op_and_the_logits_of_its_model(models, mutation):
    name = mr.MODEL_OF[mutation]
    cfg, w, refs = models[name]
    x, mask, lw, p = _layer_inputs(name, "islands")
    y, om = mr.rows_op(x, mask, lw, p)
    ym, omm = mr.rows_op(x, mask, lw, p, mutation)
    if mutation in mr.MASK_MUTATIONS:
        assert np.array_equal(y, ym) and (om != omm).sum() > 20, (mutation, int((om != omm).sum()))
    else:      # (the wrong padding side and a dropped dilation move the mask's taps with the data's)
        assert np.abs(y - ym).max() > 1e-2 and (np.array_equal(om, omm) or mutation in ("pad_left_ceil", "dilation_ignored")), mutation
    assert mr.VISIBLE_ON[mutation], mutation
    for kind in mr.KINDS:
        moved = float(np.abs(mr.forward(cfg, w, mr.ids_of(kind, N_WIN), mutation=mutation)["prediction"] - refs[kind]).max())
        if kind in mr.VISIBLE_ON[mutation]:
            assert moved > 10 * GATE, (mutation, kind, moved)
        elif kind == "full" and mutation in mr.MASK_MUTATIONS + ("input_not_masked",):
            assert moved == 0.0, (mutation, kind, moved)


def test_on_islands_the_and_differs_from_every_branch():
    for name in ("fixture", "modes"):
        x, mask, lw, p = _layer_inputs(name, "islands")
        _, om = mr.rows_op(x, mask, lw, p)
        assert 0 < om.sum() < om.size
        for b, bp in enumerate(p["branches"]):
            one = dict(merge="concat", branches=[bp])
            _, single = mr.rows_op(x, mask, {k.replace(f"branch{b}/", "branch0/"): v for k, v in lw.items() if k.startswith(f"branch{b}/")}, one)
            assert (single != om).sum() > 20 and not (om & ~single).any(), (name, b)      # the AND is below every branch's mask
    # ... and on rows without a masked position every branch's mask is full
    x, mask, lw, p = _layer_inputs("fixture", "full")
    assert mr.rows_op(x, mask, lw, p)[1].all()


# ---- (3) ----------------------------------------------------------------------------------------------------------------
def _compile(cfg, weights=None):
    from jaeger_amd import plan as P
    from jaeger_amd.program import compile_plan
    from jaeger_amd.weights import random_weights
    plan = P.build_plan(cfg)
    w = random_weights(plan) if weights is None else weights
    return plan, compile_plan(plan, w), w


def _cfg(branches=None, **over):
    cfg = load_model_cfg("multiscale500")
    return cfg if branches is None and not over else mr.with_branches(cfg, cfg["representation_learner"]["hidden_layers"][0]["config"]["branches"]
                                                                   if branches is None else branches, **over)


def test_fixture_plan_defaults_and_program():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd.program import unpack_msconv_descriptor
    cfg = _cfg()
    plan, prog, w = _compile(cfg)
    layer = plan.rep[0]
    conv = lambda b, k, f, d: P.Conv(f"rep/0/branch{b}", k, 64, f, 1, "same", d, True, None, True, "any")
    assert layer == P.MultiScaleConv("rep/0", 64, "concat", [conv(0, 3, 16, 1), conv(1, 5, 16, 1), conv(2, 3, 32, 3)])
    assert layer.channels == 64 and plan.rep_channels == 64 and plan.pooling == "average"
    assert {k: tuple(v) for k, v in P.weight_shapes(plan).items()} == {k: tuple(v) for k, v in mr.weight_specs(cfg).items()}
    # the model-level use_masking does not reach the branches (builder.py:1019-1020 names masked_conv1d, masked_batchnorm and
    # residual_block); the layer's use_bias does
    off = copy.deepcopy(cfg)
    off["use_masking"] = False
    off["representation_learner"]["hidden_layers"][0]["config"]["use_bias"] = False
    off["representation_learner"]["hidden_layers"][0]["config"]["branches"][1]["use_bias"] = True
    branches = P.build_plan(off).rep[0].branches
    assert [c.use_masking for c in branches] == [True] * 3 and [c.use_bias for c in branches] == [False, True, False]
    kinds = [op.kind for op in prog.ops]
    assert kinds == [L.OP_MASK, L.OP_CONV, L.OP_MSMASK, L.OP_MSCONV, L.OP_LOCALATTN, L.OP_LOCALATTN, L.OP_ELTWISE, L.OP_POOL, L.OP_DENSE]
    ident_mask, ident, mop, op = prog.ops[:4]
    assert ident.in_buf == L.JG_BUF_IDS and ident.k == 1 and ident.n_stages == 0 and ident.in_mask == L.JG_BUF_NONE      # the rows are not zeroed
    assert (op.cin, op.cout, op.k, op.arg) == (64, 64, 3, L.MSCONV_CONCAT) == (mop.cin, mop.cout, mop.k, mop.arg) and mop.w_off == op.w_off
    assert op.in_buf == ident.out_buf and op.out_buf not in (op.in_buf, -1) and op.in_mask == ident_mask.out_mask == mop.in_mask
    assert op.out_mask == mop.out_mask >= 0 and op.out_mask != op.in_mask and mop.in_buf == mop.out_buf == -1
    assert [op.stages[s].kind for s in range(op.n_stages)] == [L.ST_BN, L.ST_ACT]                 # the norm and the gelu ride the op's store
    la, lb, ln, pool = prog.ops[4:8]                                                               # the layers behind see the layer's mask
    assert la.in_mask == lb.in_mask == ln.out_mask == pool.in_mask == op.out_mask
    assert any("MSCONV" in row and "branches=3 merge=concat" in row for row in prog.describe())
    # the blob: the descriptor, then per branch kernel [k][cin][fpad] | bias [fpad]
    desc = unpack_msconv_descriptor(prog.blob[op.w_off:], 3)
    at = L.MSCONV_MAX_BRANCHES * L.MSCONV_DESC_FIELDS
    for b, (f, k, d, ch) in enumerate(((16, 3, 1, 0), (16, 5, 1, 16), (32, 3, 3, 32))):
        assert desc[b] == dict(filters=f, taps=k, dilation=d, activation=L.ACT_NONE, mask_mode=L.MASK_ANY, has_bias=1, channel_offset=ch, weight_offset=at)
        blob = prog.blob[op.w_off + at:op.w_off + at + (k * 64 + 1) * f]
        assert np.array_equal(blob[:k * 64 * f].reshape(k, 64, f), w[f"rep/0/branch{b}/kernel"]) and np.array_equal(blob[k * 64 * f:], w[f"rep/0/branch{b}/bias"])
        at += (k * 64 + 1) * f
    assert np.all(prog.blob[op.w_off + 24:op.w_off + 32].view(np.int32) == 0)
    # existing models compile as before
    assert not {L.OP_MSCONV, L.OP_MSMASK} & {o.kind for o in _compile(load_model_cfg("baseline500"))[1].ops}


def test_blob_of_narrow_branches_add_and_modes():
    from jaeger_amd import _lib as L
    from jaeger_amd.program import unpack_msconv_descriptor
    cfg = mr.variant("reference_small")
    plan, prog, w = _compile(cfg)
    op = [o for o in prog.ops if o.kind == L.OP_MSCONV][0]
    assert (op.cin, op.cout, op.k) == (64, 16, 2) and plan.rep[0].channels == 16
    d = unpack_msconv_descriptor(prog.blob[op.w_off:], 2)
    assert [(b["filters"], b["channel_offset"]) for b in d] == [(8, 0), (8, 8)]                   # two branches share one 16-channel block
    k0 = prog.blob[op.w_off + d[0]["weight_offset"]:][:3 * 64 * 16].reshape(3, 64, 16)             # padded to 16 columns with zeros
    assert np.array_equal(k0[..., :8], w["rep/0/branch0/kernel"]) and not k0[..., 8:].any()
    assert d[1]["weight_offset"] == d[0]["weight_offset"] + 3 * 64 * 16 + 16
    plan, prog, w = _compile(mr.variant("add"))
    op = [o for o in prog.ops if o.kind == L.OP_MSCONV][0]
    d = unpack_msconv_descriptor(prog.blob[op.w_off:], 3)
    assert (op.cout, op.arg) == (32, L.MSCONV_ADD) and plan.rep[0].channels == 32 and [b["channel_offset"] for b in d] == [0, 0, 0]
    assert [(b["activation"], b["has_bias"], b["dilation"]) for b in d] == [(L.ACT_GELU_TANH, 1, 1), (L.ACT_TANH, 0, 1), (L.ACT_RELU, 1, 2)]
    assert "rep/0/branch1/bias" not in w and not prog.blob[op.w_off + d[1]["weight_offset"] + 5 * 64 * 32:][:32].any()
    _, prog, _ = _compile(mr.variant("modes"))
    op = [o for o in prog.ops if o.kind == L.OP_MSCONV][0]
    assert [b["mask_mode"] for b in unpack_msconv_descriptor(prog.blob[op.w_off:], 3)] == [L.MASK_ANY, L.MASK_MAJORITY, L.MASK_STRICT]


def test_variants_compile_and_what_stands_behind_the_layer():
    from jaeger_amd import _lib as L
    for name in mr.VARIANTS:
        plan, prog, _ = _compile(mr.variant(name))
        kinds = [o.kind for o in prog.ops]
        masked = name not in ("behind_cross", "unmasked")
        assert kinds.count(L.OP_MSCONV) == 1 and kinds.count(L.OP_MSMASK) == int(masked), name
        at = kinds.index(L.OP_MSCONV)
        op = prog.ops[at]
        if masked:
            assert kinds[at - 1] == L.OP_MSMASK and prog.ops[at - 1].out_mask == op.out_mask        # once, in front of the mixer
        else:
            assert op.out_mask == L.JG_BUF_NONE and op.in_mask == L.JG_BUF_NONE
            assert [o for o in prog.ops if o.kind == L.OP_POOL][0].in_mask == L.JG_BUF_NONE
    _, prog, _ = _compile(mr.variant("wide"))
    op = [o for o in prog.ops if o.kind == L.OP_MSCONV][0]
    assert (op.cin, op.cout, op.k) == (128, 128, 4)
    _, prog, _ = _compile(mr.variant("ln_tail"))
    kinds = [o.kind for o in prog.ops]
    at = kinds.index(L.OP_MSCONV)
    tail = prog.ops[at + 1]
    assert prog.ops[at].n_stages == 0 and tail.kind == L.OP_ELTWISE and tail.cout == 64 and tail.out_mask == prog.ops[at].out_mask
    assert [tail.stages[s].kind for s in range(tail.n_stages)] == [L.ST_LN, L.ST_ACT]
    _, prog, _ = _compile(mr.variant("then_conv"))
    kinds = [o.kind for o in prog.ops]
    at = kinds.index(L.OP_MSCONV)
    assert kinds[at + 1:at + 3] == [L.OP_MASK, L.OP_CONV] and prog.ops[at + 1].in_mask == prog.ops[at].out_mask and prog.ops[at + 2].cin == 64
    # a residual block behind the layer (the builder hands it a stale shape that ResidualBlockStack never reads) and a standalone
    # norm further behind, which needs the channel count
    cfg = _cfg()
    layers = cfg["representation_learner"]["hidden_layers"]
    cfg["representation_learner"]["hidden_layers"] = layers[:3] + [{"name": "residual_block", "config": dict(block_size=1, filters=64, kernel_size=3)},
                                                                    {"name": "dropout", "config": {}}] + layers[3:]
    plan, prog, _ = _compile(cfg)
    assert plan.rep_channels == 64
    cfg["representation_learner"]["hidden_layers"] = layers[:1] + [layers[3], {"name": "masked_layernorm", "config": {}}]
    _, prog, _ = _compile(cfg)
    assert [o for o in prog.ops if o.kind == L.OP_ELTWISE][-1].cout == 64


def test_behind_live_dead_positions_the_masked_layer_runs_and_the_unmasked_one_is_refused():
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    unmasked = {"name": "masked_conv1d", "config": dict(filters=64, kernel_size=3, padding="same", use_masking=False)}
    cfg = _cfg()
    layers = cfg["representation_learner"]["hidden_layers"]
    ms2 = copy.deepcopy(layers[0])
    cfg["representation_learner"]["hidden_layers"] = layers[:4] + [ms2, unmasked] + layers[4:]      # behind the masked layer no dead position is live
    cfg["representation_learner"]["pooling"] = "average"
    plan = P.build_plan(cfg)
    G.compile_plan(plan, random_weights(plan))
    for b in ms2["config"]["branches"]:
        b["use_masking"] = False
    plan = P.build_plan(cfg)
    with pytest.raises(P.UnsupportedLayer, match="multi_scale_conv whose branches do not mask.*reads masked positions unmasked"):
        G.compile_plan(plan, random_weights(plan))


# ---- (4) ----------------------------------------------------------------------------------------------------------------
B3 = dict(filters=32, kernel_size=3)


@pytest.mark.parametrize("branches, over, word", [
    ([], {}, "branches must be a non-empty list of dicts"),
    ([B3, "x"], {}, "branches must be a non-empty list of dicts"),
    ({"a": B3}, {}, "branches must be a non-empty list of dicts"),
    ([B3, B3], dict(merge="mul"), "merge must be 'concat' or 'add', got 'mul'"),
    ([B3, dict(filters=16, kernel_size=3)], dict(merge="add"), "All branches must have the same filters when merge='add'"),
    ([B3, dict(B3, padding="valid")], {}, "Branch 1: padding must be 'same' to keep sequence length aligned across branches, got 'valid'"),
    ([dict(B3, strides=2), B3], {}, "Branch 0: strides must be 1 to keep sequence length aligned across branches, got 2"),
    ([B3, dict(B3, mask_mode="most")], {}, r"Invalid mask_mode: 'most' \(use 'any', 'majority' or 'strict'\)"),
])
def test_refused_as_the_reference_raises(branches, over, word):
    from jaeger_amd import plan as P
    with pytest.raises(ValueError, match=word) as err:
        P.build_plan(_cfg(branches, **over))
    assert not isinstance(err.value, P.UnsupportedLayer)


@pytest.mark.parametrize("branches, over, word", [
    ([B3, dict(B3, axis=1)], {}, "branch 1: axis 1 .*axis = -1"),
    ([B3, dict(B3, use_masking=False)], {}, "branches disagree on use_masking .*ANDs a branch's mask with None"),
    ([B3, dict(B3, groups=2)], {}, r"branch 1: \['groups'\] are no arguments of MaskedConv1D"),
    ([B3] * 5, {}, "5 branches .*1 to 4"),
    ([dict(filters=12, kernel_size=3), dict(filters=20, kernel_size=3)], {}, "branch 0: filters 12 .*multiple of 8 up to 128"),
    ([dict(filters=136, kernel_size=3)], {}, "branch 0: filters 136"),
    ([B3, dict(filters=32, kernel_size=16)], {}, "branch 1: kernel_size 16 .*1 to 15"),
    ([dict(filters=64, kernel_size=3, dilation_rate=33)], {}, r"branch 0: \(kernel_size - 1\) x dilation_rate = 66 .*up to 64"),
    ([dict(filters=64, kernel_size=15, dilation_rate=5)], {}, r"\(kernel_size - 1\) x dilation_rate = 70"),
    ([dict(filters=8, kernel_size=3)], {}, "8 output channels .*multiple of 16 up to 128"),
    ([dict(filters=16, kernel_size=3), dict(filters=8, kernel_size=3)], {}, "24 output channels"),
    ([dict(filters=96, kernel_size=3), dict(filters=48, kernel_size=3)], {}, "144 output channels"),
])
def test_refused_with_the_reason_that_names_the_limit(branches, over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_cfg(branches, **over))


def test_refused_widths_heads_strands_nmd_taps_and_the_generic_fall_through():
    from jaeger_amd import plan as P
    for width in (24, 144):
        cfg = _cfg()
        cfg["embedding"]["embedding_size"] = width
        with pytest.raises(P.UnsupportedLayer, match=f"{width} incoming channels .*multiple of 16 up to 128"):
            P.build_plan(cfg)
    ms = _cfg()["representation_learner"]["hidden_layers"][0]
    cfg = _cfg()
    cfg["classifier"]["hidden_layers"].insert(0, copy.deepcopy(ms))
    with pytest.raises(P.UnsupportedLayer, match="multi_scale_conv.*head or on a strand branch"):
        P.build_plan(cfg)
    cfg = load_model_cfg("dvf500")
    cfg["representation_learner"]["branch"]["hidden_layers"].insert(1, copy.deepcopy(ms))
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"][1]["config"]["return_nmd"] = True
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind multi_scale_conv"):
        P.build_plan(cfg)
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"].insert(1, {"name": "nmd", "config": {}})
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind multi_scale_conv"):
        P.build_plan(cfg)
    # an entry without `branches`, or with a key that is none of the constructor's arguments: the generic refusal
    for bad in ({}, dict(merge="concat"), dict(branches=[B3, B3], filters=64), dict(branches=[B3, B3], padding="same"),
                dict(embed_dim=32, num_heads=4, feed_forward_dim=64)):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"][0]["config"] = dict(bad)
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)
    # ... and the training-only keys are taken
    P.build_plan(_cfg(None, kernel_initializer="he_normal", kernel_regularizer="l2", kernel_regularizer_w=1e-5, use_bias=False))


# ---- (5) ----------------------------------------------------------------------------------------------------------------
def test_weight_names_and_shapes():
    from jaeger_amd import plan as P
    shapes = {k: v for k, v in P.weight_shapes(P.build_plan(mr.variant("add"))).items() if k.startswith("rep/0/")}
    assert shapes == {"rep/0/branch0/kernel": (3, 64, 32), "rep/0/branch0/bias": (32,), "rep/0/branch1/kernel": (5, 64, 32),
                      "rep/0/branch2/kernel": (3, 64, 32), "rep/0/branch2/bias": (32,)}


def test_h5_bundle_and_verify_model_refuse_and_name_the_npz_route(tmp_path):
    from click.testing import CliRunner

    import yaml
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.cli import main
    from jaeger_amd.verify import verify_model
    cfg = load_model_cfg("multiscale500")
    cfg["representation_learner"]["hidden_layers"] = cfg["representation_learner"]["hidden_layers"][:3]      # (the layer alone names itself)
    plan = P.build_plan(cfg)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"multi_scale_conv.*weights\.npz"):
        W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"multi_scale_conv.*weights\.npz"):
        W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
    with pytest.raises(P.UnsupportedLayer, match=r"verify-model does not cover multi_scale_conv.*weights\.npz"):
        verify_model(tmp_path / "m_graph", plan)
    cfg = load_model_cfg("multiscale500")
    plan = P.build_plan(cfg)
    w = W.random_weights(plan)
    assert set(w) == set(mr.weight_specs(cfg)) and all(w[k].shape == tuple(v) for k, v in mr.weight_specs(cfg).items())
    W.save_npz(tmp_path / "multiscale500.weights.npz", w)
    back = W.load_weights({"weights_npz": tmp_path / "multiscale500.weights.npz"}, plan)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    (tmp_path / "g").mkdir()
    (tmp_path / "p.yaml").write_text(yaml.safe_dump({"model": cfg}))
    res = CliRunner().invoke(main, ["verify-model", str(tmp_path / "g"), "--project", str(tmp_path / "p.yaml")])
    assert res.exit_code != 0 and "multi_scale_conv" in res.output and "weights.npz" in res.output


def test_abi_symbols_and_constants():
    from jaeger_amd import _lib as L
    lib = L.load()
    assert lib.jg_msconv_tile() == L.MSCONV_TILE == mr.TILE
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    enum = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", header).group(1))
    assert enum("JG_OP_MSCONV") == L.OP_MSCONV == 18 and enum("JG_OP_MSMASK") == L.OP_MSMASK == 19
    assert lib.jg_sizeof(0) == ctypes.sizeof(L.JgOp)
    kernel_header = (ROOT / "jaeger_amd" / "csrc" / "jg_msconv.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", kernel_header).group(1))
    assert define("JG_MSCONV_TILE") == L.MSCONV_TILE and define("JG_MSCONV_MAX_BRANCHES") == L.MSCONV_MAX_BRANCHES
    assert define("JG_MSCONV_DESC_FIELDS") == L.MSCONV_DESC_FIELDS and (define("JG_MSCONV_CONCAT"), define("JG_MSCONV_ADD")) == (L.MSCONV_CONCAT, L.MSCONV_ADD)


# ---- (6) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture", "add", "modes"])
def test_emulation_stays_close_to_the_restatement(name):
    for kind in ("ragged", "islands"):
        x, mask, lw, p = _layer_inputs(name, kind)
        x, mask = x[:12], mask[:12]
        want, _ = mr.rows_op(x, mask, lw, p)
        emu = mr.emulate(x, lw, p, mask)
        e, r = ar.errors(emu, want)
        assert emu.dtype == np.float32 and e <= 1e-5 and r <= 1e-5, (name, kind, e, r)
