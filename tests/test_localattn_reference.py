"""Local attention on the CPU tier (the GPU tier is tests/test_gpu_localattn.py):

(1) the float64 restatement of ``LocalAttention`` (tests/local_attention_reference.py) against torch's own multi-head
    attention under the additive -1e9 mask, at every live position;
(2) the host-side fold, evaluated plainly, equals the restatement;
(3) a numpy emulation of the kernel's arithmetic sets the per-op bound (a power of two at or above 4 x its own error
    against the restatement, element and RMS error in units of the output's RMS);
(4) every mutation - the bugs such a kernel typically has - lies outside that bound on the input kinds named for it; where
    a mutation cannot show on a kind it is printed as invisible there (pytest -s);
(5) the fixture model (crossframe500 with its attention layer swapped for local_attention) -> plan -> program, the
    refusals, the weight loaders;
(6) the new symbols and constants of the C-ABI.
"""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_reference as ar
import local_attention_reference as lr
from conftest import ROOT, load_model_cfg

#: channels / heads / feed-forward width / half-window
SIZES = {"16/2/32/8": (16, 2, 32, 8), "32/4/128/8": (32, 4, 128, 8), "64/8/256/32": (64, 8, 256, 32), "32/4/128/0": (32, 4, 128, 0)}
LENGTHS = (5, 17, 160)


def _window(half):
    return 2 * half if half else 1


def _block(size, seed=3):
    c, h, f, half = SIZES[size]
    rng = np.random.Generator(np.random.PCG64(seed))
    return ar.random_layer_weights(lr.block_specs(c, h, f), rng), c, h, _window(half)


def _row_masks(l, half):
    """Four rows: all valid; right-padded from the middle on; one invalid run longer than 2 half + 1 (as long as the row
    allows); one shorter run."""
    m = np.ones((4, l), bool)
    m[1, (l + 1) // 2:] = False
    long_run = min(2 * half + 4, l - 2)
    a = max((l - long_run) // 2, 1)
    m[2, a:a + long_run] = False
    m[3, 1:1 + max(min(half, l - 2), 1)] = False
    return m


# ---- (1) ----------------------------------------------------------------------------------------------------------------
def test_restatement_against_torch():
    seen_dead = seen_masked_live = 0
    for size in SIZES:
        w, c, h, window = _block(size)
        d, half = c // h, window // 2
        t = lambda name: torch.as_tensor(np.asarray(w[name], np.float64))
        for l in LENGTHS:
            x = np.random.Generator(np.random.PCG64(l)).normal(0, 1, (4, l, c)).astype(np.float32)
            mask = _row_masks(l, half)
            x64 = torch.as_tensor(x.astype(np.float64))
            tok = x64.permute(1, 0, 2)                                            # (L tokens, rows, C): sequence first
            xn = F.layer_norm(tok, (c,), t("ln1/gamma"), t("ln1/beta"), 1e-6)
            in_w = torch.cat([t(f"mha/{p}/kernel").reshape(c, h * d).T for p in ("query", "key", "value")])
            in_b = torch.cat([t(f"mha/{p}/bias").reshape(h * d) for p in ("query", "key", "value")])
            q, k = np.arange(l)[:, None], np.arange(l)[None, :]
            allowed = (np.abs(q - k) <= half)[None] & mask[:, None, :]            # M[r, q, k]
            add = torch.as_tensor(np.where(allowed, 0.0, -1e9)).repeat_interleave(h, dim=0)      # (rows * heads, L, L)
            out, _ = F.multi_head_attention_forward(
                xn, xn, xn, c, h, in_w, in_b, None, None, False, 0.0, t("mha/attention_output/kernel").reshape(h * d, c).T,
                t("mha/attention_output/bias"), training=False, need_weights=False, attn_mask=add)
            y = tok + out
            yn = F.layer_norm(y, (c,), t("ln2/gamma"), t("ln2/beta"), 1e-6)
            y = y + F.gelu(yn @ t("ffn1/kernel") + t("ffn1/bias"), approximate="tanh") @ t("ffn2/kernel") + t("ffn2/bias")
            want = y.permute(1, 0, 2).numpy()
            got, dead = lr.local_attention_block(x, w, h, window, mask)
            assert np.array_equal(dead, ~allowed.any(axis=-1))
            live = ~dead
            assert live.any(), (size, l)
            seen_dead += int(dead.sum())
            seen_masked_live += int((live & ~mask).sum())
            assert (got[dead] == 0.0).all()
            elem, rms = lr.live_errors(got, want, dead)
            at_dead = float(np.abs(got - want)[dead].max()) if dead.any() else 0.0
            print(f"{size:12s} L {l:3d}: live {int(live.sum()):4d} (masked {int((live & ~mask).sum()):3d}), dead {int(dead.sum()):3d}; "
                  f"restatement vs torch float64 at live positions: max {elem:.2e}, rms {rms:.2e}; torch's value at dead ones is off by {at_dead:.2g}")
            assert elem <= 1e-12, (size, l, elem)
    assert seen_dead > 0 and seen_masked_live > 0


def test_no_mask_means_the_band_alone_and_blocks_share_the_mask():
    w, c, h, window = _block("32/4/128/8")
    x = np.random.Generator(np.random.PCG64(1)).normal(0, 1, (2, 30, c)).astype(np.float32)
    y, dead = lr.local_attention_block(x, w, h, window, None)
    y1, dead1 = lr.local_attention_block(x, w, h, window, np.ones((2, 30), bool))
    assert not dead.any() and np.array_equal(y, y1)
    x2 = x.copy()
    x2[:, 20:] = x[:, 20:][:, ::-1] * 1.5                      # position 11 sees keys 3 .. 19 only (half-window 8)
    assert np.array_equal(lr.local_attention_block(x2, w, h, window, None)[0][:, :12], y[:, :12])
    assert np.abs(lr.local_attention_block(x2, w, h, window, None)[0][:, 12] - y[:, 12]).max() > 1e-6
    # window_size 1: every position attends itself alone
    z, _ = lr.local_attention_block(x, w, h, 1, None)
    z2, _ = lr.local_attention_block(x[:, ::-1], w, h, 1, None)
    assert np.allclose(z2[:, ::-1], z, rtol=0, atol=1e-13)


# ---- (2) ----------------------------------------------------------------------------------------------------------------
#: the fold rounds every folded weight to f32 once (2^-24 relative each); C + F of them meet in an output element with
#: random signs: 2^-20 of the output's RMS is three bits above the 2.5e-7 this measures
FOLD_BOUND = 2.0 ** -20


@pytest.mark.parametrize("size", list(SIZES))
def test_fold_evaluated_plainly_is_the_restatement(size):
    w, c, h, window = _block(size)
    fw = lr.fold(w, h)
    for l in (17, 40):
        x = np.random.Generator(np.random.PCG64(l)).normal(0, 1, (4, l, c)).astype(np.float32)
        mask = _row_masks(l, window // 2)
        want, dead = lr.local_attention_block(x, w, h, window, mask)
        got = lr.evaluate_fold(x, fw, h, window, mask)
        e, r = lr.live_errors(got, want, dead)
        print(f"{size:12s} L {l}: folded operands vs restatement: max {e:.2e}, rms {r:.2e}")
        assert e <= FOLD_BOUND and (got[dead] == 0).all()


# ---- (3) ----------------------------------------------------------------------------------------------------------------
#: as in tests/test_frameattn_reference.py: a broken emulation would set a useless bound; its own error must stay where
#: f32 arithmetic puts it (offset rows: 2^-24 x 60 x 20 ~ 7e-5 of a unit-scale output)
EMULATION_SANITY = 2.0 ** -12


@pytest.mark.parametrize("size", list(SIZES))
def test_emulation_sets_the_bound(size):
    w, c, h, window = _block(size)
    l = 40
    mask = lr.window_ids(l, "ragged", n_win=1, half=window // 2).reshape(6, l) != 0
    for name, x in lr.value_inputs(c, 6, l):
        ref, dead = lr.local_attention_block(x, w, h, window, mask)
        emu = lr.emulate_block(x, w, h, window, mask)
        b = lr.bounds_from(emu, ref, dead)
        print(f"{size:12s} {name:12s} emulation: max {b['emu_elem']:.3g} rms {b['emu_rms']:.3g} -> bound max 2^{int(np.log2(b['elem']))} "
              f"= {b['elem']:.3g}, rms 2^{int(np.log2(b['rms']))} = {b['rms']:.3g}")
        assert b["elem"] >= ar.HEADROOM * b["emu_elem"] and b["rms"] >= ar.HEADROOM * b["emu_rms"]
        assert b["emu_elem"] < EMULATION_SANITY, "the emulation itself is off"
        assert (emu[dead] == 0).all() and (dead.any() or window // 2 > 8)      # (half-window 32 reaches every padded position of 40)


# ---- (4) ----------------------------------------------------------------------------------------------------------------
def test_every_mutation_lies_outside_its_bound():
    c, h, f, half = SIZES["32/4/128/8"]
    window, blocks, l = 16, 2, 40
    w = ar.random_layer_weights(lr.layer_specs(c, h, f, blocks), np.random.Generator(np.random.PCG64(3)))
    x = lr.value_inputs(c, 12, l)[0][1].reshape(2, 6, l, c)
    shown = {m: [] for m in lr.MUTATIONS}
    for kind in lr.KINDS:
        mask = lr.window_ids(l, kind, n_win=2, half=half) != 0
        ref, dead = lr.local_attention(x, w, h, window, blocks, mask)
        b = lr.bounds_from(lr.emulate(x, w, h, window, blocks, mask), ref, dead)
        print(f"{kind}: {int(dead.sum())} dead, {int((~mask & ~dead).sum())} masked but live positions; bound max {b['elem']:.3g}, rms {b['rms']:.3g}")
        for m in lr.MUTATIONS:
            e, r = lr.live_errors(lr.local_attention(x, w, h, window, blocks, mask, mutation=m)[0], ref, dead)
            margin = max(e / b["elem"], r / b["rms"])
            required = kind in lr.VISIBLE_ON[m]
            print(f"    {margin:12.3g}x  {m:34s} {'' if required else ('invisible on this kind' if margin <= 1 else '(not required on this kind)')}")
            if required:
                assert margin > 1.0, (m, kind, margin)
                shown[m].append(kind)
    for m, kinds in shown.items():
        assert kinds, f"{m} is visible on no input kind"


# ---- (5) ----------------------------------------------------------------------------------------------------------------
def _cfg(**over):
    return lr.fixture_cfg(load_model_cfg("crossframe500"), **over)


def _compile(cfg):
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    plan = P.build_plan(cfg)
    return plan, G.compile_plan(plan, random_weights(plan))


def test_fixture_compiles_to_two_local_attention_ops_that_keep_the_mask():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    cfg = _cfg()
    plan = P.build_plan(cfg)
    att = [l for l in plan.rep if isinstance(l, P.LocalAttn)]
    assert len(att) == 1 and (att[0].channels, att[0].heads, att[0].key_dim, att[0].ff_dim, att[0].half_window, att[0].blocks) == (32, 4, 8, 128, 8, 2)
    assert {n: tuple(s) for n, s in P.weight_shapes(plan).items()} == {n: tuple(s) for n, s in lr.weight_specs(cfg).items()}
    w = lr.random_weights(cfg)
    prog = G.compile_plan(plan, w)
    at = [i for i, op in enumerate(prog.ops) if op.kind == L.OP_LOCALATTN]
    assert len(at) == 2 and at[1] == at[0] + 1
    a, b = prog.ops[at[0]], prog.ops[at[1]]
    for op in (a, b):
        assert (op.cin, op.cout, op.k, op.arg, op.stride, op.dilation) == (32, 32, 4, 128, 8, 1) and abs(op.f0 - 1e-6) < 1e-12
        assert op.in_buf != op.out_buf and op.in_mask >= 0 and op.out_mask == op.in_mask
    assert b.in_buf == a.out_buf and b.out_buf != a.out_buf and b.in_mask == a.in_mask
    assert a.n_stages == 0 and [b.stages[s].kind for s in range(b.n_stages)] == [L.ST_BN]     # the norm rides the LAST block's store
    pool = [o for o in prog.ops if o.kind == L.OP_POOL][0]
    assert pool.in_buf == b.out_buf and pool.in_mask == b.in_mask                              # the mask is kept behind the layer
    assert any("LOCALATTN" in row and "heads=4 ff=128 half_window=8" in row for row in prog.describe())
    # the packed weights are the fold the emulation restates, bit for bit, per block
    for j, op in enumerate((a, b)):
        want = lr.blob_of(lr.fold(ar.sub_weights(w, f"{att[0].name}/block{j}"), 4))
        assert np.array_equal(prog.blob[op.w_off:op.w_off + want.size], want)
    # existing models compile as before: no local-attention op, the frame-attention op where it was
    base = G.compile_plan(P.build_plan(load_model_cfg("crossframe500")), ar.random_weights(load_model_cfg("crossframe500")))
    assert [op.kind for op in base.ops].count(L.OP_FRAMEATTN) == 1 and L.OP_LOCALATTN not in [op.kind for op in base.ops]


def test_no_mask_behind_cross_frame_attention_and_one_block():
    from jaeger_amd import _lib as L
    cfg = load_model_cfg("crossframe500")
    cfg["representation_learner"]["hidden_layers"].insert(7, {"name": lr.LOCAL, "config": dict(lr.FIXTURE, num_blocks=1, window_size=1)})
    _, prog = _compile(cfg)
    op = [o for o in prog.ops if o.kind == L.OP_LOCALATTN]
    assert len(op) == 1 and op[0].in_mask == L.JG_BUF_NONE and op[0].out_mask == L.JG_BUF_NONE and op[0].stride == 0


def test_tail_stages_the_store_cannot_carry_become_ops_behind_it():
    from jaeger_amd import _lib as L
    for norm, lead in (("masked_layernorm", L.ST_LN), ("masked_dyt", L.ST_DYT)):
        cfg = _cfg()
        layers = cfg["representation_learner"]["hidden_layers"]
        layers[-1] = {"name": norm, "config": {}}
        layers.append({"name": "activation", "config": {"activation": "gelu"}})
        _, prog = _compile(cfg)
        kinds = [op.kind for op in prog.ops]
        at = max(i for i, k in enumerate(kinds) if k == L.OP_LOCALATTN)
        assert prog.ops[at].n_stages == 0 and kinds[at + 1] == L.OP_ELTWISE
        tail = prog.ops[at + 1]
        assert [tail.stages[s].kind for s in range(tail.n_stages)] == [lead, L.ST_ACT] and tail.stages[0].arg == 1
        assert tail.out_mask == prog.ops[at].out_mask and tail.in_buf == tail.out_buf == prog.ops[at].out_buf


@pytest.mark.parametrize("over, word", [
    (dict(embed_dim=64), "embed_dim 64 != 32 incoming channels"),
    (dict(num_heads=3), "num_heads 3"),
    (dict(num_heads=16), "key_dim"),
    (dict(feed_forward_dim=512), "feed_forward_dim 512"),
    (dict(feed_forward_dim=100), "feed_forward_dim 100"),
    (dict(feed_forward_dim=0), "feed_forward_dim 0"),
    (dict(window_size=0), "window_size 0"),
    (dict(window_size=66), "window_size 66"),
    (dict(num_blocks=0), "num_blocks 0"),
])
def test_plan_refusals_name_the_limit(over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_cfg(**over))


def test_plan_refuses_other_widths_heads_branches_and_incomplete_entries():
    from jaeger_amd import plan as P
    cfg = _cfg(embed_dim=48)
    for layer in cfg["representation_learner"]["hidden_layers"]:
        if "filters" in layer["config"]:
            layer["config"]["filters"] = 48
    with pytest.raises(P.UnsupportedLayer, match="embed_dim 48 .*16 / 32 / 64"):
        P.build_plan(cfg)
    P.build_plan(_cfg(window_size=65))                                    # half-window 32: the largest the kernel covers
    cfg = load_model_cfg("crossframe500")
    cfg["classifier"]["hidden_layers"].insert(0, {"name": lr.LOCAL, "config": dict(lr.FIXTURE)})
    with pytest.raises(P.UnsupportedLayer, match="local_attention.*head or on a strand branch"):
        P.build_plan(cfg)
    cfg = load_model_cfg("dvf500")
    cfg["representation_learner"]["branch"]["hidden_layers"].insert(1, {"name": lr.LOCAL, "config": dict(lr.FIXTURE)})
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)
    for missing in ("embed_dim", "num_heads", "feed_forward_dim", "window_size"):      # the reference's constructor raises too
        cfg = _cfg()
        layer = [l for l in cfg["representation_learner"]["hidden_layers"] if l["name"] == lr.LOCAL][0]
        del layer["config"][missing]
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)
    for other in ("axial_attention", "transformer_encoder", "multi_scale_conv"):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"][6] = {"name": other, "config": dict(lr.FIXTURE)}
        with pytest.raises(P.UnsupportedLayer, match="outside the Conv1D"):
            P.build_plan(cfg)


def test_compiler_refuses_what_would_read_dead_positions_and_what_it_cannot_place():
    from jaeger_amd import plan as P
    conv = lambda **kw: {"name": "masked_conv1d", "config": dict(filters=32, kernel_size=3, padding="same", **kw)}
    res = lambda **kw: {"name": "residual_block", "config": dict(filters=32, kernel_size=3, **kw)}
    cross = {"name": ar.ATTN, "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=128)}
    for extra, over, word in ((conv(use_masking=False), {}, "conv without masking"),
                              (res(use_masking=False), {}, "residual block without masking"),
                              (cross, {}, "cross_frame_attention"),
                              ({"name": "masked_batchnorm", "config": dict(use_masking=False)}, {}, "use_masking: false"),
                              (res(), dict(window_size=1), "output mask grows by 2 positions")):
        cfg = _cfg(**over)
        cfg["representation_learner"]["hidden_layers"].append(extra)
        with pytest.raises(P.UnsupportedLayer, match=word) as err:
            _compile(cfg)
        assert "local_attention" in str(err.value) and "reads masked positions unmasked" in str(err.value)
    # the readers that mask compile: a masked conv, a masked residual block inside the band's reach, the masked norms, nmd
    for extra in ([conv()], [res()], [conv(), res(use_masking=True), {"name": "nmd", "config": {}}],
                  [{"name": "masked_layernorm", "config": {}}], [conv(), cross]):
        cfg = _cfg()
        cfg["representation_learner"]["hidden_layers"] += extra
        _compile(cfg)
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"][7]["config"]["return_nmd"] = True
    with pytest.raises(P.UnsupportedLayer, match="nmd tap directly behind local_attention"):
        _compile(cfg)
    cfg = _cfg()
    cfg["representation_learner"]["hidden_layers"] = cfg["representation_learner"]["hidden_layers"][6:]
    cfg["embedding"]["embedding_size"] = 32
    with pytest.raises(P.UnsupportedLayer, match="local_attention directly on the embedding"):
        _compile(cfg)


def test_h5_bundle_and_verify_model_refuse_and_name_the_npz_route(tmp_path):
    from click.testing import CliRunner

    import yaml
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.cli import main
    from jaeger_amd.verify import verify_model
    cfg = _cfg()
    plan = P.build_plan(cfg)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"local_attention.*weights\.npz"):
        W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"local_attention.*weights\.npz"):
        W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
    with pytest.raises(P.UnsupportedLayer, match=r"verify-model does not cover local_attention.*weights\.npz"):
        verify_model(tmp_path / "m_graph", plan)
    w = W.random_weights(plan)
    assert set(w) == set(lr.weight_specs(cfg))
    W.save_npz(tmp_path / "m.weights.npz", w)
    back = W.load_weights({"weights_npz": tmp_path / "m.weights.npz"}, plan)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    (tmp_path / "g").mkdir()
    (tmp_path / "p.yaml").write_text(yaml.safe_dump({"model": cfg}))
    res = CliRunner().invoke(main, ["verify-model", str(tmp_path / "g"), "--project", str(tmp_path / "p.yaml")])
    assert res.exit_code != 0 and "local_attention" in res.output and "weights.npz" in res.output


# ---- (6) ----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_constants():
    from jaeger_amd import _lib as L
    lib = L.load()
    assert lib.jg_localattn_tile() == L.LOCALATTN_TILE == 80
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    enum = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", header).group(1))
    assert enum("JG_OP_LOCALATTN") == L.OP_LOCALATTN == L.OP_FRAMEATTN + 1
    assert enum("JG_PROF_LOCALATTN") == L.JG_PROF_LOCALATTN and enum("JG_PROF_LOCALATTN_CVT") == L.JG_PROF_LOCALATTN_CVT
    assert enum("JG_PROF_CLASSES") == L.JG_PROF_LOCALATTN_CVT + 1
    assert lib.jg_sizeof(0) == ctypes.sizeof(L.JgOp)
    from jaeger_amd import plan as P
    assert P.LOCALATTN_MAX_HALF == L.LOCALATTN_MAX_HALF == 32
    kernel_header = (ROOT / "jaeger_amd" / "csrc" / "jg_localattn.h").read_text()
    assert re.search(r"#define JG_LOCALATTN_TILE (\d+)", kernel_header).group(1) == "80"
    assert re.search(r"#define JG_LOCALATTN_MAX_HALF (\d+)", kernel_header).group(1) == "32"
