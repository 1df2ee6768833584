"""``parallel_branches`` of pooled branches and last pooling on the CPU (the GPU tier is tests/test_gpu_branches.py).

1. the restated poolers and merges (tests/branches_reference.py) against an independent torch formulation - ``torch.gather``
   for last, ``torch.stack(...).sum / mean / amax`` for the merges - to 1e-12;
2. the plan: widths, names, dropped taps, ``pooling is None``; the weights and the loaders that refuse;
3. the program: the POOLVEC ops' kinds, merges, offsets and scales, every branch's first op on the trunk's slot, slots given
   back, branches on the trunk's dead-position state; every existing golden project still compiles to one ``JG_OP_POOL``;
4. every refusal, with the reference's wording where it is the reference's;
5. seven mutations of the reference against the unmutated one on the GPU test's windows: each moves the logits of its model
   by at least 8 x the 1e-4 gate on at least one window kind (the table is printed);
6. the float32 emulation of the op's sum order against the restatement; the ABI constants.
"""
import copy
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import branches_reference as xr
from conftest import GOLDEN, load_model_cfg

ROOT = Path(__file__).resolve().parents[1]
GATE = 1e-4


def _compile(cfg, weights=None):
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    plan = P.build_plan(cfg)
    weights = xr.random_weights(cfg) if weights is None else weights
    return plan, G.compile_plan(plan, weights), weights


def _poolvecs(prog):
    from jaeger_amd import _lib as L
    return [i for i, op in enumerate(prog.ops) if op.kind == L.OP_POOLVEC]


# ---- (1) ------------------------------------------------------------------------------------------------------------------
def _tensor(seed=3, b=4, f=6, l=23, c=8):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = torch.as_tensor(rng.normal(0, 1, (b, f, l, c)))
    m = rng.random((b, f, l)) < 0.7
    m[0] = True                       # a full window
    m[1, 2] = False                   # one empty frame
    m[2] = False                      # an empty window
    m[3, :, l // 2:] = False          # trailing padding ...
    m[3, 1, 3:7] = False              # ... and a run inside: count - 1 is not the last valid index
    return x, torch.as_tensor(m.astype(np.float64))


def test_poolers_against_an_independent_formulation():
    x, m = _tensor()
    b, f, l, c = x.shape
    mb = m != 0
    # last: torch.gather at count - 1, zeros for empty frames, the sum over max(frames with a valid position, 1)
    count = mb.sum(-1)
    idx = (count - 1).clamp(min=0)
    g = torch.gather(x, 2, idx[:, :, None, None].expand(b, f, 1, c))[:, :, 0]
    g = torch.where((count > 0)[..., None], g, torch.zeros_like(g))
    want = g.sum(1) / (count > 0).sum(1).clamp(min=1)[:, None]
    assert (xr.pool_last(x, m) - want).abs().max() <= 1e-12
    assert not xr.pool_last(x, m)[2].any()
    assert (xr.pool_last(x, None) - x[:, :, l - 1].mean(1)).abs().max() <= 1e-12
    # the run inside: the count rule and the docstring's rule differ, and the position read is itself masked
    assert count[3, 1] - 1 != torch.nonzero(mb[3, 1]).max() and not mb[3, 1, count[3, 1] - 1]
    assert (xr.pool_last(x, m) - xr.pool_last(x, m, "last_index_of_last_valid"))[3].abs().max() > 1e-3
    # max: positions as one axis, -1e9 where masked, zeros for the empty window; average: sum over count
    flat, fm = x.reshape(b, f * l, c), mb.reshape(b, f * l)
    want = torch.where(fm[..., None], flat, torch.full_like(flat, -1.0e9)).amax(1)
    want[~fm.any(1)] = 0.0
    assert (xr.pool_max(x, m) - want).abs().max() <= 1e-12
    want = (flat * fm[..., None]).sum(1) / fm.sum(1).clamp(min=1e-7)[:, None]
    assert (xr.pool_average(x, m) - want).abs().max() <= 1e-12
    assert (xr.pool_max(x, None) - flat.amax(1)).abs().max() <= 1e-12 and (xr.pool_average(x, None) - flat.mean(1)).abs().max() <= 1e-12


def test_merges_against_an_independent_formulation():
    rng = np.random.Generator(np.random.PCG64(5))
    vs = [torch.as_tensor(rng.normal(0, 1, (4, 8))) for _ in range(3)]
    st = torch.stack(vs)
    assert (xr.merge(vs, "sum") - st.sum(0)).abs().max() <= 1e-12
    assert (xr.merge(vs, "average") - st.mean(0)).abs().max() <= 1e-12
    assert (xr.merge(vs, "max") - st.amax(0)).abs().max() <= 1e-12
    assert torch.equal(xr.merge(vs, "concat"), torch.cat(vs, -1))
    assert torch.equal(xr.merge(vs[:1], "average"), vs[0])
    with pytest.raises(ValueError, match="Unknown parallel_branches merge method: mul"):
        xr.merge(vs, "mul")
    with pytest.raises(ValueError, match="incompatible shapes"):
        xr.merge([vs[0], vs[1][:, :4]], "sum")


# ---- (2) ------------------------------------------------------------------------------------------------------------------
def test_fixture_plan():
    from jaeger_amd import plan as P
    cfg = xr.fixture_cfg()
    plan = P.build_plan(cfg)
    assert plan.pooling is None and plan.rep_channels == 64 and plan.nmd_dims == [] and plan.reliability is None
    node = plan.rep[-1]
    assert isinstance(node, P.ParallelBranches) and node.name == "rep/3" and node.merge == "concat" and node.channels == 64
    assert [(b.pooling, b.channels, [type(l).__name__ for l in b.layers]) for b in node.branches] == [("max", 32, ["ResBlock"])] * 2
    assert [b.layers[0].name for b in node.branches] == ["rep/3/branch0/0/block0", "rep/3/branch1/0/block0"]
    assert [b.layers[0].conv1.dilation_rate for b in node.branches] == [2, 6]
    assert plan.classifier[0].cin == 64


@pytest.mark.parametrize("name", list(xr.VARIANTS))
def test_variants_plan_widths_names_and_programs(name):
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    cfg = xr.variant(name)
    plan, prog, weights = _compile(cfg)
    shapes = P.weight_shapes(plan)
    assert set(shapes) == set(weights) == set(xr.weight_specs(cfg))
    assert all(tuple(weights[k].shape) == tuple(v) for k, v in shapes.items())
    assert plan.nmd_dims == [] and not prog.has_reliability and prog.nmd_dim == 0
    pv = [prog.ops[i] for i in _poolvecs(prog)]
    at = xr.branches_at(cfg)
    n_pool = sum(op.kind == L.OP_POOL for op in prog.ops)
    assert not any(op.kind in (L.OP_NMD_FINAL,) or any(op.stages[s].kind == L.ST_NMD for s in range(op.n_stages)) for op in prog.ops)
    if at is None:
        assert plan.pooling == "last" and n_pool == 0 and len(pv) == 1
        op = pv[0]
        assert (op.arg, op.k, op.vec_off, op.cout, op.f0, op.out_vec) == (L.POOL_LAST, L.POOLVEC_STORE, 0, plan.rep_channels, 1.0, L.VEC_EMBEDDING)
        return
    entry = cfg["representation_learner"]["hidden_layers"][at]["config"]
    widths, how, n = xr.branch_widths(cfg), entry["merge"], len(entry["branches"])
    assert plan.pooling is None and n_pool == 0 and len(pv) == n
    assert plan.rep_channels == xr.merged_width(cfg) == prog.embedding_dim == (sum(widths) if how == "concat" else widths[0])
    off = 0
    for b, (op, bcfg) in enumerate(zip(pv, entry["branches"])):
        kind = {"max": L.POOL_MAX, "average": L.POOL_AVG, "last": L.POOL_LAST}[xr.POOLINGS[bcfg["pooling"]]]
        merge = L.POOLVEC_STORE if how == "concat" or b == 0 else L.POOLVEC_MAX if how == "max" else L.POOLVEC_ADD
        scale = np.float32(1.0 / n) if how == "average" and b == n - 1 else np.float32(1.0)
        assert (op.arg, op.k, op.vec_off, op.cout, op.out_vec) == (kind, merge, off, widths[b], L.VEC_EMBEDDING), (name, b)
        assert np.float32(op.f0) == scale
        off += widths[b] if how == "concat" else 0


def test_program_branches_read_the_trunk_and_give_their_slots_back():
    from jaeger_amd import _lib as L
    cfg = xr.variant("four_branches")
    plan, prog, _ = _compile(cfg)
    pv = _poolvecs(prog)
    trunk = prog.ops[pv[0] - 4 - 1]                       # the trunk's closing element-wise op (layer norm + gelu), in place
    assert trunk.kind == L.OP_ELTWISE and trunk.in_buf == trunk.out_buf
    tbuf, tmask = trunk.out_buf, trunk.out_mask
    start = pv[0] - 4
    used_bufs, used_masks = set(), set()
    for b, end in enumerate(pv):
        ops = prog.ops[start:end + 1]
        assert [o.kind for o in ops] == [L.OP_MASK, L.OP_CONV, L.OP_MASK, L.OP_CONV, L.OP_POOLVEC], b
        assert ops[0].in_mask == tmask and ops[1].in_buf == tbuf and ops[1].in_mask == tmask, f"branch {b} does not start on the trunk"
        assert ops[3].stages[[ops[3].stages[s].kind for s in range(ops[3].n_stages)].index(L.ST_ADD)].arg == tbuf      # the shortcut
        for o in ops[:4]:
            assert o.out_buf != tbuf and o.out_mask != tmask, f"branch {b} writes a slot of the trunk"
        assert ops[4].in_buf == ops[3].out_buf and ops[4].in_mask == ops[3].out_mask
        used_bufs |= {o.out_buf for o in ops[:4] if o.out_buf >= 0}
        used_masks |= {o.out_mask for o in ops[:4] if o.out_mask >= 0}
        start = end + 1
    # every branch got the same slots again: nothing leaks from branch to branch (four branches, six slots)
    assert len(used_bufs) == 2 and len(used_masks) == 2, (used_bufs, used_masks)
    assert max(used_bufs | {tbuf}) < L.JG_MAX_BUFS


def test_branch_that_needs_too_many_slots_gets_the_existing_refusal(monkeypatch):
    """The trunk's slot stays taken while a branch runs: with four slots the fixture's branches fit (trunk, conv1, conv2), and
    a branch with a bypass conv (one slot more, next to the held one) meets the slot allocator's own refusal."""
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    assert L.JG_MAX_BUFS == 6
    bypass = xr.branches_cfg([xr._branch([xr._resblock(2, use_1x1conv=True)])])
    _compile(bypass)
    monkeypatch.setattr(L, "JG_MAX_BUFS", 3)
    _compile(xr.fixture_cfg())
    with pytest.raises(P.UnsupportedLayer, match="program needs more than 3 activation buffers"):
        _compile(bypass)


def test_every_branch_starts_from_the_trunks_dead_position_state():
    """Behind a local_attention whose zeroed positions are live: a masked conv branch clears the state for itself only - the
    ``last`` pool of the NEXT branch, which reads the trunk's tensor unmasked, is still refused; with the branches swapped the
    refusal names branch 0."""
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    local = {"name": "local_attention", "config": dict(embed_dim=32, num_heads=4, feed_forward_dim=64, window_size=16)}
    conv = xr._branch([xr._CONV16 | {"config": dict(xr._CONV16["config"], filters=32)}], "last")
    bare = xr._branch([], "last")
    for branches, word in (([conv, bare], "branch1"), ([bare, conv], "branch0")):
        plan = P.build_plan(xr.branches_cfg(branches, trunk_extra=[local], width=64))
        with pytest.raises(P.UnsupportedLayer, match=rf"{word}: pooling: last .*behind rep/3 \(local_attention\)"):
            G.compile_plan(plan, random_weights(plan))
    plan = P.build_plan(xr.branches_cfg([conv, xr._branch([], "max")], trunk_extra=[local], width=64))      # a masked reader: fine
    G.compile_plan(plan, random_weights(plan))
    cfg = load_model_cfg("hyena500")                       # top-level last behind a live local_attention
    rep = cfg["representation_learner"]
    rep["hidden_layers"] = rep["hidden_layers"][:3] + [local]
    rep["pooling"] = "last"
    plan = P.build_plan(cfg)
    with pytest.raises(P.UnsupportedLayer, match=r"pooling: last .*reads masked positions unmasked"):
        G.compile_plan(plan, random_weights(plan))


def test_existing_golden_projects_keep_their_single_pool_op():
    from jaeger_amd import _lib as L
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    names = sorted(p.name[:-len("_project.yaml")] for p in GOLDEN.glob("*_project.yaml"))
    assert "brain" in names and "branches500" in names and len(names) > 5
    for name in names:
        if name == "branches500":
            continue
        plan = P.build_plan(load_model_cfg(name))
        prog = G.compile_plan(plan, random_weights(plan))
        kinds = [op.kind for op in prog.ops]
        assert kinds.count(L.OP_POOLVEC) == 0 and kinds.count(L.OP_POOL) == 1, (name, kinds)
        assert plan.pooling in ("max", "average", "max1d", "average1d")


# ---- (4) ------------------------------------------------------------------------------------------------------------------
R2, R6 = xr._resblock(2), xr._resblock(6)


def _with_entry(**config):
    cfg = xr.fixture_cfg()
    cfg["representation_learner"]["hidden_layers"][xr.branches_at(cfg)]["config"] = config
    return cfg


def _top_pooling(pooling):
    cfg = xr.fixture_cfg()
    cfg["representation_learner"]["pooling"] = pooling
    return cfg


UNEQUAL = [xr._branch([R2]), xr._branch([xr._CONV16])]          # 32 + 16 channels: fine under concat (the variant "unequal")


@pytest.mark.parametrize("cfg, word", [
    (_with_entry(merge="concat", branches=[]), "^parallel_branches requires at least one branch$"),
    (_with_entry(merge="concat"), "^parallel_branches requires at least one branch$"),
    (_with_entry(merge="mul", branches=[xr._branch([R2])]), "^Unknown parallel_branches merge method: mul$"),
    (_with_entry(merge="sum", branches=UNEQUAL), r"merge 'sum' over branches of unequal width \[32, 16\]"),
    (_with_entry(merge="average", branches=UNEQUAL), r"merge 'average' over branches of unequal width \[32, 16\]"),
    (_with_entry(merge="max", branches=UNEQUAL), r"merge 'max' over branches of unequal width \[32, 16\]"),
    (_top_pooling("max"), "pooling 'max' behind a parallel_branches of pooled branches.*must be null"),
    (_top_pooling("last"), "pooling 'last' behind a parallel_branches of pooled branches.*must be null"),
])
def test_refused_as_the_reference_fails(cfg, word):
    from jaeger_amd import plan as P
    with pytest.raises(ValueError, match=word) as err:
        P.build_plan(cfg)
    assert not isinstance(err.value, P.UnsupportedLayer)


def _nested():
    inner = {"name": xr.BRANCHES, "config": {"merge": "concat", "branches": [xr._branch([R2])]}}
    return xr._branch([inner])


@pytest.mark.parametrize("branches, over, word", [
    ([{"hidden_layers": [R2]}], {}, "branch0: a branch without pooling .*Keras' merge layers"),
    ([{"hidden_layers": [R2], "pooling": None}, {"hidden_layers": [R6], "pooling": None}], {}, "branch0: a branch without pooling"),
    ([xr._branch([R2]), {"hidden_layers": [R6]}], {}, "mixes pooled and unpooled branches"),
    ([xr._branch([R2], "gatedframe")], {}, "branch0: pooling 'gatedframe' in a branch"),
    ([xr._branch([R2], "median")], {}, r"branch0: pooling 'median' is not supported \(max / average / last\)"),
    ([_nested()], {}, "nested parallel_branches"),
    ([xr._branch([xr._resblock(d)]) for d in (1, 2, 3, 4, 5)], {}, r"5 branches \(up to 4\)"),
    ([xr._branch([xr._resblock(2, filters=30, use_1x1conv=True)])], {}, "branch0: a branch of 30 channels .*multiple of 4"),
    ([xr._branch([xr._resblock(2, filters=512, use_1x1conv=True)]) for _ in range(3)], {}, "leaves 1536 channels .*up to 1024"),
    ([xr._branch([R2])], {"axis": -1}, r"parallel_branches keys \['axis'\]"),
    ([dict(xr._branch([R2]), name="b0")], {}, r"branch0: branch keys \['name'\]"),
])
def test_refused_with_the_reason(branches, over, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_with_entry(merge="concat", branches=copy.deepcopy(branches), **over))


def test_refused_behind_the_merge_in_heads_on_strands_and_gated_at_the_top():
    from jaeger_amd import plan as P
    from jaeger_amd import program as G
    from jaeger_amd.weights import random_weights
    entry = xr.fixture_cfg()["representation_learner"]["hidden_layers"][3]
    cfg = xr.fixture_cfg()
    cfg["representation_learner"]["hidden_layers"].append({"name": "dropout", "config": {"rate": 0.1}})
    P.build_plan(cfg)                                      # dropout behind the merge is taken
    for behind in ({"name": "activation", "config": {"activation": "gelu"}}, {"name": "dense", "config": {"units": 8}},
                   {"name": "masked_batchnorm", "config": {}}):
        cfg = xr.fixture_cfg()
        cfg["representation_learner"]["hidden_layers"].append(behind)
        with pytest.raises(P.UnsupportedLayer, match="behind a parallel_branches of pooled branches .*only dropout"):
            P.build_plan(cfg)
    cfg = xr.fixture_cfg()
    cfg["classifier"]["hidden_layers"].insert(0, copy.deepcopy(entry))
    with pytest.raises(P.UnsupportedLayer, match="parallel_branches .*head or on a strand branch"):
        P.build_plan(cfg)
    cfg = load_model_cfg("dvf500")
    cfg["representation_learner"]["branch"]["hidden_layers"].insert(1, copy.deepcopy(entry))
    with pytest.raises(P.UnsupportedLayer):
        P.build_plan(cfg)
    cfg = xr.fixture_cfg()
    cfg["representation_learner"]["pooling"] = "gatedframe"
    with pytest.raises(ValueError):
        P.build_plan(cfg)
    cfg = load_model_cfg("hyena500")
    cfg["representation_learner"]["pooling"] = "gatedframe"
    with pytest.raises(P.UnsupportedLayer, match=r"pooling 'gatedframe' is not supported \(max / average / last\)"):
        P.build_plan(cfg)
    # a reliability head on a model whose taps are all dropped: the reference's own error
    cfg = xr.variant("taps_dropped")
    cfg["reliability_model"] = copy.deepcopy(load_model_cfg("brain")["reliability_model"])
    with pytest.raises(ValueError, match="produced no NMD tensor"):
        P.build_plan(cfg)
    # a norm / activation as a branch's first layer would run in place on the trunk's tensor
    plan = P.build_plan(xr.branches_cfg([xr._branch([{"name": "activation", "config": {"activation": "relu"}}, R2]), xr._branch([R6])]))
    with pytest.raises(P.UnsupportedLayer, match="first layer of a branch .*in place"):
        G.compile_plan(plan, random_weights(plan))


def test_h5_bundle_and_verify_model_refuse_and_name_the_npz_route(tmp_path):
    from click.testing import CliRunner

    import yaml
    from jaeger_amd import plan as P
    from jaeger_amd import weights as W
    from jaeger_amd.cli import main
    from jaeger_amd.verify import verify_model
    cfg = xr.fixture_cfg()
    plan = P.build_plan(cfg)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"parallel_branches.*weights\.npz"):
        W.load_keras3_h5(tmp_path / "m.weights.h5", plan)
    with pytest.raises(W.AttentionWeightsUnsupported, match=r"parallel_branches.*weights\.npz"):
        W.load_savedmodel_bundle(tmp_path / "m_graph", plan)
    with pytest.raises(P.UnsupportedLayer, match=r"verify-model does not cover parallel_branches.*weights\.npz"):
        verify_model(tmp_path / "m_graph", plan)
    w = W.random_weights(plan)
    assert set(w) == set(xr.weight_specs(cfg)) and all(w[k].shape == tuple(v) for k, v in xr.weight_specs(cfg).items())
    assert {"rep/3/branch0/0/block0/conv1/kernel", "rep/3/branch1/0/block0/bn2/moving_variance"} <= set(w)
    W.save_npz(tmp_path / "branches500.weights.npz", w)
    back = W.load_weights({"weights_npz": tmp_path / "branches500.weights.npz"}, plan)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    (tmp_path / "g").mkdir()
    (tmp_path / "p.yaml").write_text(yaml.safe_dump({"model": cfg}))
    res = CliRunner().invoke(main, ["verify-model", str(tmp_path / "g"), "--project", str(tmp_path / "p.yaml")])
    assert res.exit_code != 0 and "parallel_branches" in res.output and "weights.npz" in res.output


# ---- (5) ------------------------------------------------------------------------------------------------------------------
#: mutation -> the model it is held on.  The two ``last`` mutations cannot reach the fixture's logits (it pools by max): that
#: is asserted, and they are held on the siblings with last pooling
#: the window kinds the shifts are measured on: the three that carry invalid positions of the three shapes (a run inside a row,
#: an empty frame, an empty window); ``full`` and ``tail_n`` add nothing to them
MUTATION_KINDS = ("long_n", "empty_row", "empty_window")
MUTATION_MODELS = {
    "last_index_of_last_valid": ("pool_last",),
    "last_divides_by_all_frames": ("pool_last",),
    "average_not_divided": ("merge_average",),
    "sum_for_max": ("merge_max",),
    "concat_swapped": ("fixture",),
    "branch_chain": ("fixture",),
    "branch_mask_dropped": ("fixture", "pool_last"),
}


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(name):
        if name not in cache:
            cfg = xr.variant(name)
            w = xr.random_weights(cfg)
            cache[name] = (cfg, w, {k: xr.forward(cfg, w, xr.ids_of(k))["prediction"] for k in MUTATION_KINDS})
        return cache[name]
    return get


def test_every_mutation_moves_the_logits_of_its_model(references):
    assert set(MUTATION_MODELS) == set(xr.MUTATIONS)
    rows, failed = [], []
    for mutation, names in MUTATION_MODELS.items():
        for name in names:
            cfg, w, refs = references(name)
            shift = {k: float(np.abs(xr.forward(cfg, w, xr.ids_of(k), mutation=mutation)["prediction"] - refs[k]).max())
                     for k in MUTATION_KINDS}
            rows.append(f"{mutation:28s} {name:14s} " + "  ".join(f"{k} {v:.2e}" for k, v in shift.items()))
            if max(shift.values()) < 8 * GATE:
                failed.append(rows[-1])
    print("\nlargest logit shift per mutation, model and window kind (gate 1e-4):")
    for row in rows:
        print("  " + row)
    assert not failed, failed
    cfg, w, refs = references("fixture")
    for mutation in ("last_index_of_last_valid", "last_divides_by_all_frames", "average_not_divided", "sum_for_max"):
        for k in ("long_n", "empty_row"):
            got = xr.forward(cfg, w, xr.ids_of(k), mutation=mutation)["prediction"]
            assert np.array_equal(got, refs[k]), f"{mutation} reaches the fixture's logits"


def test_window_kinds_hold_what_they_are_for():
    l = xr.ids_of("full").shape[2]
    assert (xr.ids_of("full") != 0).all() and xr.ids_of("full").shape == (xr.N_WIN, 6, l)
    cfg = xr.variant("pool_last")
    info = {}
    xr.forward(cfg, xr.random_weights(cfg), xr.ids_of("long_n"), info=info)
    for b in (0, 1):                                       # behind BOTH branches' convs a run survives inside a row
        _, m = info[b]
        count = m.sum(-1)
        last = np.where(m.any(-1), m.shape[-1] - 1 - m[..., ::-1].argmax(-1), -1)
        assert ((count - 1 != last) & (count > 0)).any(), f"branch {b}: count - 1 is the last valid index everywhere"
        rows = np.argwhere((count - 1 != last) & (count > 0))
        assert any(not m[w_, f_, count[w_, f_] - 1] for w_, f_ in rows), f"branch {b}: the position read is valid everywhere"
    ids = xr.ids_of("empty_row")
    assert not ids[0, 2].any() and not ids[-1, 5].any() and ids[0, 0].any()
    ids = xr.ids_of("empty_window")
    assert not ids[1].any() and ids[0].any() and ids[2].any()
    ids = xr.ids_of("tail_n")
    assert (ids[:, :, 0] != 0).all() and (ids[:, :, -1] == 0).any()
    out = xr.forward(cfg, xr.random_weights(cfg), xr.ids_of("empty_window"))
    assert not out["embedding"][1].any()


# ---- (6) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["max", "average", "last"])
def test_emulation_stays_close_to_the_restatement(kind):
    for c, l in ((32, 23), (20, 7), (64, 1)):              # 256 / (c / 4) whole and not whole; fewer positions than groups
        x, m = _tensor(seed=c, l=l, c=c)
        x = x.to(torch.float32)
        mb = m.numpy() != 0
        for mask in (m, None):
            want = xr.pool(x.to(torch.float64), mask, kind).numpy()
            emu = xr.emulate_pool(x.numpy(), None if mask is None else mb, kind)
            assert emu.dtype == np.float32 and emu.shape == want.shape
            if kind == "max":
                np.testing.assert_array_equal(emu, want.astype(np.float32))
            else:
                assert np.abs(emu - want).max() <= 2.0 ** -20 * max(np.abs(want).max(), 1.0), (kind, c, l)
    vs = [np.float32(np.arange(8) * s) for s in (1.0, -0.5, 0.25)]
    np.testing.assert_array_equal(xr.emulate_merge(vs, "average"), ((vs[0] + vs[1]) + vs[2]) * np.float32(1.0 / 3.0))
    np.testing.assert_array_equal(xr.emulate_merge(vs, "max"), np.maximum(np.maximum(vs[0], vs[1]), vs[2]))
    assert xr.emulate_merge(vs, "concat").shape == (24,)


def test_abi_symbols_and_constants():
    from jaeger_amd import _lib as L
    lib = L.load()
    header = (ROOT / "include" / "jaeger_hip.h").read_text()
    enum = lambda name: int(re.search(rf"\b{name}\s*=\s*(\d+)", header).group(1))
    assert enum("JG_OP_POOLVEC") == L.OP_POOLVEC == 20 and enum("JG_OP_MSMASK") == L.OP_MSMASK == 19 and enum("JG_OP_POOL") == L.OP_POOL == 3
    assert (enum("JG_POOL_MAX"), enum("JG_POOL_AVG"), enum("JG_POOL_LAST")) == (L.POOL_MAX, L.POOL_AVG, L.POOL_LAST) == (0, 1, 3)
    assert (enum("JG_POOLVEC_STORE"), enum("JG_POOLVEC_ADD"), enum("JG_POOLVEC_MAX")) == (L.POOLVEC_STORE, L.POOLVEC_ADD, L.POOLVEC_MAX)
    assert lib.jg_sizeof(0) == ctypes.sizeof(L.JgOp) and lib.jg_abi_version() == 1
    kernel_header = (ROOT / "jaeger_amd" / "csrc" / "jg_poolvec.h").read_text()
    from jaeger_amd import plan as P
    assert int(re.search(r"#define JG_POOLVEC_MAX_WIDTH (\d+)", kernel_header).group(1)) == L.POOLVEC_MAX_WIDTH == P.BRANCHES_MAX_WIDTH
    assert "jg_poolvec.hip" in (ROOT / "jaeger_amd" / "csrc" / "Makefile").read_text()
