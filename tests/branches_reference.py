"""Reference side of the ``parallel_branches`` / last-pooling checks (tests/test_branches_reference.py on the CPU,
tests/test_gpu_branches.py on the GPU): a float64 restatement of how the reference turns the representation tensor into the
embedding vector - ``nnlib/builder.py:1109-1153`` (every branch a block of its own on the same tensor and mask, the pooled
vectors merged in branch order) and ``MaskedLastPooling`` (``nnlib/v2/layers.py:541-578``).  Nothing here imports the product.

The trunk and the branches run through ``oracle.forward._run_block``; a ``hyena_block``, ``masked_bilstm`` or
``multi_scale_conv`` among them through its own reference module, composed as tests/mixer_reference.py composes them.  What
this module adds:

* the three poolers (:func:`pool_max`, :func:`pool_average`, :func:`pool_last`) and the four merges (:func:`merge`);
* MaskedLastPooling as its CODE has it, not its docstring: ``idx = (valid positions of the frame row) - 1`` - the count, not
  the index of the last valid position; the value at ``max(idx, 0)`` whatever its mask bit; frames with ``idx < 0`` add
  zeros; the sum over the frames divided by ``max(frames with idx >= 0, 1)``; without a mask the mean over the frames of the
  last position;
* the dropped taps: NMD taps inside a branch are built and dropped (builder.py:1124-1125), and with ``pooling: null`` the
  block returns the tensor alone (:1169-1193), so taps in the trunk are dropped too - such a model has no ``nmd`` output;
* ``forward(..., mutation=)``: one of :data:`MUTATIONS`, each a plausible misreading.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import attention_reference as ar
import bilstm_reference as br
import hyena_reference as hr
import local_attention_reference as lr
import multiscale_reference as mr
from attention_reference import f32
from conftest import load_model_cfg
from oracle import forward as of

BRANCHES = "parallel_branches"
MIXERS = (hr.HYENA, br.BILSTM, mr.MSCONV)
FSIZE = 500
# by how many positions the layers in front of a pool shorten an invalid run (mask mode "any": a conv's output is valid where
# any tap is): the trunk's 7-tap conv by 6, a 5-tap residual block of dilation 6 by 2 x 24
GROW = 54
N_WIN = 3
WINDOW_KINDS = ("full", "long_n", "tail_n", "empty_row", "empty_window")
POOLINGS = {"max": "max", "masked_max": "max", "average": "average", "masked_average": "average", "last": "last",
            "masked_last": "last"}
MERGES = ("concat", "sum", "average", "max")

MUTATIONS = (
    "last_index_of_last_valid",      # pool_last: idx = the index of the last valid position (what the docstring says)
    "last_divides_by_all_frames",    # pool_last: the divisor ignores that a frame is all-masked and counts every frame
    "average_not_divided",           # merge average: the running sum alone
    "sum_for_max",                   # merge max: the sum
    "concat_swapped",                # merge concat: the offsets of the first two branches swapped
    "branch_chain",                  # branch 1 is fed branch 0's output tensor and mask, not the trunk's
    "branch_mask_dropped",           # the last branch runs and pools without the incoming mask
)


# ---- the poolers and the merges -------------------------------------------------------------------------------------------
def pool_max(x, mask):
    """MaskedGlobalMaxPooling (layers.py:517-529) over (frames, length): x (B, F, L, C), mask (B, F, L) of 0 / 1 or None."""
    return of.masked_global_max(x, mask)


def pool_average(x, mask):
    """MaskedGlobalAvgPooling (layers.py:460-480)."""
    return of.masked_global_avg(x, mask)


def pool_last(x, mask, mutation: str | None = None):
    """MaskedLastPooling.call (layers.py:556-569), line by line."""
    b, f, l, c = x.shape
    if mask is None:
        return x[:, :, -1, :].mean(dim=1)
    m = (mask != 0).to(torch.int64)
    idx = m.sum(dim=-1) - 1                                              # the COUNT minus one
    if mutation == "last_index_of_last_valid":
        pos = torch.arange(l).expand(b, f, l)
        idx = torch.where(m != 0, pos, torch.full_like(pos, -1)).amax(dim=-1)
    safe = torch.clamp(idx, min=0)
    rows = x.reshape(b * f, l, c)
    gathered = rows[torch.arange(b * f), safe.reshape(-1)].reshape(b, f, c)
    valid = (idx >= 0).to(x.dtype)
    gathered = gathered * valid[..., None]
    count = torch.clamp(valid.sum(dim=1, keepdim=True), min=1.0)
    if mutation == "last_divides_by_all_frames":
        count = torch.full_like(count, float(f))
    return gathered.sum(dim=1) / count


def pool(x, mask, pooling: str, mutation: str | None = None):
    kind = POOLINGS[str(pooling).lower()]
    return pool_max(x, mask) if kind == "max" else pool_average(x, mask) if kind == "average" else pool_last(x, mask, mutation)


def merge(vectors: list, how: str, mutation: str | None = None):
    """Concatenate / Add / Average / Maximum over the branch vectors, in branch order (builder.py:1128-1141)."""
    if how == "concat":
        if mutation == "concat_swapped" and len(vectors) > 1:
            vectors = [vectors[1], vectors[0]] + list(vectors[2:])
        return torch.cat(list(vectors), dim=-1)
    if how not in MERGES:
        raise ValueError(f"Unknown parallel_branches merge method: {how}")
    if len({tuple(v.shape) for v in vectors}) != 1:
        raise ValueError(f"Inputs have incompatible shapes: {[tuple(v.shape) for v in vectors]}")
    out = vectors[0]
    for v in vectors[1:]:
        out = torch.maximum(out, v) if how == "max" and mutation != "sum_for_max" else out + v
    if how == "average" and mutation != "average_not_divided":
        out = out / len(vectors)
    return out


# ---- the models -----------------------------------------------------------------------------------------------------------
def fixture_cfg() -> dict:
    return load_model_cfg("branches500")


def _resblock(d: int, filters: int = 32, **over) -> dict:
    return {"name": "residual_block", "config": dict(dict(use_1x1conv=False, block_size=1, filters=filters, kernel_size=5,
                                                          dilation_rate=d, use_bias=True), **over)}


def _branch(layers: list, pooling: str = "max") -> dict:
    return {"hidden_layers": copy.deepcopy(layers), "pooling": pooling}


def branches_cfg(branches: list, merge_: str = "concat", trunk_extra: list | None = None, width: int | None = None) -> dict:
    """The fixture with its branches replaced; ``trunk_extra``: layers put between the trunk's gelu and the branches; ``width``:
    the merged width, where the layers are none this module can size."""
    cfg = fixture_cfg()
    rep = cfg["representation_learner"]
    at = branches_at(cfg)
    entry = {"name": BRANCHES, "config": {"merge": merge_, "branches": copy.deepcopy(branches)}}
    rep["hidden_layers"] = rep["hidden_layers"][:at] + copy.deepcopy(trunk_extra or []) + [entry]
    cfg["classifier"]["input_shape"] = merged_width(cfg) if width is None else width
    return cfg


def last_cfg(name: str) -> dict:
    """An existing fixture (``hyena500``, ``bilstm500``) with ``pooling: last``."""
    cfg = load_model_cfg(name)
    cfg["representation_learner"]["pooling"] = "last"
    return cfg


_MSCONV_ENTRY = {"name": mr.MSCONV, "config": {"branches": [dict(filters=16, kernel_size=3), dict(filters=16, kernel_size=5, dilation_rate=2)],
                                               "merge": "concat"}}
_HYENA_ENTRY = {"name": hr.HYENA, "config": {"dim": 32, "order": 2}}
_CONV16 = {"name": "masked_conv1d", "config": dict(filters=16, kernel_size=5, padding="same", dilation_rate=3)}

VARIANTS = {
    "fixture": lambda: fixture_cfg(),
    "one_branch": lambda: branches_cfg([_branch([_resblock(2)])]),
    "three_branches": lambda: branches_cfg([_branch([_resblock(2)]), _branch([_resblock(6)]), _branch([_resblock(1)])]),
    "four_branches": lambda: branches_cfg([_branch([_resblock(d)]) for d in (1, 2, 4, 6)]),
    "merge_sum": lambda: branches_cfg([_branch([_resblock(2)]), _branch([_resblock(6)]), _branch([_resblock(1)])], "sum"),
    "merge_average": lambda: branches_cfg([_branch([_resblock(2)]), _branch([_resblock(6)]), _branch([_resblock(1)])], "average"),
    "merge_max": lambda: branches_cfg([_branch([_resblock(2)], "average"), _branch([_resblock(6)], "average"), _branch([], "average")], "max"),
    "unequal": lambda: branches_cfg([_branch([_resblock(2)]), _branch([_CONV16])]),
    "pool_average": lambda: branches_cfg([_branch([_resblock(2)], "average"), _branch([_resblock(6)], "masked_average")]),
    "pool_last": lambda: branches_cfg([_branch([_resblock(2)], "last"), _branch([_resblock(6)], "masked_last")]),
    "hyena_last": lambda: branches_cfg([_branch([_HYENA_ENTRY], "last"), _branch([_resblock(2)], "max")]),
    "msconv_branch": lambda: branches_cfg([_branch([_MSCONV_ENTRY, {"name": "masked_batchnorm", "config": {}}], "average"),
                                            _branch([_resblock(6)], "max")]),
    "taps_dropped": lambda: branches_cfg([_branch([_resblock(2, return_nmd=True)]), _branch([_resblock(6)]),],
                                         trunk_extra=[{"name": "nmd", "config": {}}]),
    "hyena500_last": lambda: last_cfg("hyena500"),
    "bilstm500_last": lambda: last_cfg("bilstm500"),
}


def variant(name: str) -> dict:
    return VARIANTS[name]()


def branches_at(cfg: dict) -> int | None:
    """The index of the ``parallel_branches`` entry among the representation learner's layers, None without one."""
    for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"]):
        if str(layer.get("name", "")).lower() == BRANCHES:
            return i
    return None


def ids_of(kind: str, n_win: int = N_WIN, l: int | None = None) -> np.ndarray:
    """(n_win, 6, l) codon ids at FSIZE.  ``full``: no invalid id.  ``long_n``: in every row of the even (window + frame) sums a
    run of invalid ids long enough to outlast the convs in front of the pool, so that ``count - 1`` is NOT the index of the
    last valid position (and the position it names may itself be invalid).  ``tail_n``: trailing padding of a different
    length per window and frame.  ``empty_row``: ``tail_n`` with one frame of window 0 and one of the last window all
    invalid.  ``empty_window``: ``tail_n`` with every frame of window 1 all invalid."""
    from oracle import encoder as oenc
    l = oenc.frame_length(FSIZE) if l is None else l
    assert kind in WINDOW_KINDS, kind
    if kind == "full":
        return ar.window_ids(l, "full", n_win, 17)
    if kind == "long_n":
        return lr.window_ids(l, "long_n", n_win=n_win, seed=17, half=8, grow=GROW)
    rng = np.random.Generator(np.random.PCG64(23))
    ids = rng.integers(1, 65, (n_win, 6, l))
    for w in range(n_win):
        for f in range(6):
            ids[w, f, int(rng.integers(l // 2, l + 1)):] = 0
    if kind == "empty_row":
        ids[0, 2] = 0
        ids[n_win - 1, 5] = 0
    if kind == "empty_window":
        ids[min(1, n_win - 1)] = 0
    return ids.astype(np.uint8)


# ---- weights --------------------------------------------------------------------------------------------------------------
def _mixers_of(layers: list) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {})) for i, layer in enumerate(layers)
            if str(layer.get("name", "")).lower() in MIXERS]


def _mixer_specs(kind: str, a: dict, cin: int) -> tuple[dict[str, tuple], int]:
    if kind == hr.HYENA:
        return hr._specs_of(kind, a), cin
    if kind == br.BILSTM:
        return br.layer_specs(cin, int(a["units"])), 2 * int(a["units"])
    p = mr.params_of(a)
    return mr.layer_specs(cin, p), mr.out_channels(p)


_PAD = {"name": "dropout", "config": {}}


def _without_taps(layers: list) -> list:
    """The layers as the graph keeps them where the taps are dropped: an ``nmd`` layer is no part of it."""
    return [_PAD if str(layer.get("name", "")).lower() == "nmd" else layer for layer in layers]


def _layer_specs(prefix: str, layers: list, cin: int, specs: dict, mixers: dict) -> int:
    """``oracle.forward._block_specs`` over a layer list that may hold the three mixers; returns the channels behind it."""
    start = 0
    for cut, kind, a in _mixers_of(layers) + [(len(layers), "", {})]:
        cin = of._block_specs(prefix, [_PAD] * start + list(layers[start:cut]), cin, specs, [])
        if kind:
            own, cin = _mixer_specs(kind, a, cin)
            mixers[f"{prefix}/{cut}"] = kind
            for leaf, shp in own.items():
                specs[f"{prefix}/{cut}/{leaf}"] = shp
        start = cut + 1
    return cin


def _rep_specs(cfg: dict, specs: dict, mixers: dict) -> tuple[int, list[int]]:
    """The representation learner's variables; returns (the embedding vector's width, the branch widths)."""
    emb = cfg["embedding"]
    assert emb.get("use_embedding_layer", False)
    cin = int(emb["embedding_size"])
    specs["embedding/embeddings"] = (of.vocab_size(cfg), cin)
    layers = cfg["representation_learner"]["hidden_layers"]
    at = branches_at(cfg)
    if at is None:
        return _layer_specs("rep", layers, cin, specs, mixers), []
    assert at == len(layers) - 1
    cin = _layer_specs("rep", _without_taps(layers[:at]), cin, specs, mixers)
    entry = layers[at]["config"]
    widths = [_layer_specs(f"rep/{at}/branch{b}", _without_taps(bcfg.get("hidden_layers", [])), cin, specs, mixers)
              for b, bcfg in enumerate(entry["branches"])]
    return (sum(widths) if entry.get("merge", "concat") == "concat" else widths[0]), widths


def merged_width(cfg: dict) -> int:
    return _rep_specs(cfg, {}, {})[0]


def branch_widths(cfg: dict) -> list[int]:
    return _rep_specs(cfg, {}, {})[1]


def weight_specs(cfg: dict, mixers: dict | None = None) -> dict[str, tuple]:
    specs: dict[str, tuple] = {}
    width, _ = _rep_specs(cfg, specs, {} if mixers is None else mixers)
    of._block_specs("classifier", cfg["classifier"]["hidden_layers"], width, specs)
    return specs


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    """Seeded stand-in weights by the rules of ``mixer_reference.random_weights``: He-uniform kernels, a bilstm's own scales,
    hyena's by its module's ``random_layer_weights``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mixers: dict[str, str] = {}
    specs = weight_specs(cfg, mixers)
    own = lambda name: next((kind for top, kind in mixers.items() if name.startswith(top + "/")), None)
    out = {}
    for name, shp in sorted(specs.items()):
        leaf = name.rsplit("/", 1)[1]
        kind = own(name)
        if kind == hr.HYENA:
            continue
        if leaf == "recurrent_kernel":
            lim = math.sqrt(3.0 / shp[0])
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "kernel" and kind == br.BILSTM:
            lim = math.sqrt(6.0 / (shp[0] + shp[1] // 4))
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "kernel":
            lim = math.sqrt(6.0 / int(np.prod(shp[:-1])))
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "embeddings":
            v = rng.normal(0.0, 1.0 / math.sqrt(shp[1]) * 4.0, shp)
        elif leaf in ("gamma", "moving_variance"):
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.normal(0.0, 0.1, shp)
            if kind == br.BILSTM:
                v[shp[0] // 4:shp[0] // 2] += 1.0
        out[name] = v.astype(f32)
    for top, kind in mixers.items():
        if kind == hr.HYENA:
            sub = {k[len(top) + 1:]: s for k, s in specs.items() if k.startswith(top + "/")}
            for leaf, v in hr.random_layer_weights(sub, rng).items():
                out[f"{top}/{leaf}"] = v
    return out


# ---- the forward ----------------------------------------------------------------------------------------------------------
def run_layers(x, mask, layers: list, prefix: str, weights: dict, cfg: dict, dtype):
    """``layers`` on the tensor ``x`` (B, F, L, C) under ``mask`` (B, F, L) or None; returns the tensor and the mask behind them.
    The conv family through ``oracle.forward._run_block`` (its taps dropped), the mixers through their own modules, the
    hand-over of the mask as in tests/mixer_reference.py."""
    start = 0
    for cut, kind, a in _mixers_of(layers) + [(len(layers), "", {})]:
        seg = [_PAD] * start + _without_taps(list(layers[start:cut]))
        x, _ = of._run_block(x, mask, seg, prefix, weights, cfg, dtype)
        mask = lr._mask_behind(mask, seg, cfg, dtype)
        if not kind:
            break
        lw = ar.sub_weights(weights, f"{prefix}/{cut}")
        xn = x.detach().numpy()
        b_, fr, l, c = xn.shape
        mk = None if mask is None else mask.numpy() != 0
        rows = lambda t: None if t is None else t.reshape((b_ * fr, l) + t.shape[3:])
        if kind == hr.HYENA:
            y = hr.hyena_block(rows(xn), lw, rows(mk), **hr.params_of(a)).reshape(b_, fr, l, c)
        elif kind == br.BILSTM:
            p = br.params_of(a)
            y = np.asarray(br.bilstm(rows(xn), lw, rows(mk), p["ignore_mask"]), np.float64).reshape(b_, fr, l, 2 * p["units"])
            if p["ignore_mask"]:
                mask = None
        else:
            y, mask = mr.multi_scale_conv(x, mask, lw, mr.params_of(a), None, dtype)
        x = torch.as_tensor(np.asarray(y)).to(dtype) if not torch.is_tensor(y) else y.to(dtype)
        start = cut + 1
    return x, mask


def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64, mutation: str | None = None,
            info: dict | None = None) -> dict[str, np.ndarray]:
    """ids (W, 6, L) -> {"embedding", "prediction"} in float64.  ``mutation``: one of MUTATIONS.  ``info``: a dict that
    receives, per branch (or under ``"top"`` for a model without branches), the tensor and the mask the pool read."""
    assert mutation is None or mutation in MUTATIONS, mutation
    idt = torch.as_tensor(np.asarray(ids).astype(np.int64))
    emb_cfg = cfg["embedding"]
    assert emb_cfg.get("use_embedding_layer", False) and not emb_cfg.get("use_positional_embeddings", False)
    x = torch.as_tensor(weights["embedding/embeddings"]).to(dtype)[idt]
    mask = (idt != 0).to(dtype)
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    at = branches_at(cfg)
    keep = (lambda key, t, m: None) if info is None else \
        (lambda key, t, m: info.__setitem__(key, (t.detach().numpy(), None if m is None else m.numpy() != 0)))
    if at is None:
        x, mask = run_layers(x, mask, layers, "rep", weights, cfg, dtype)
        keep("top", x, mask)
        vec = pool(x, mask, rep["pooling"], mutation)
    else:
        assert at == len(layers) - 1 and rep.get("pooling") is None
        x, mask = run_layers(x, mask, layers[:at], "rep", weights, cfg, dtype)
        entry = layers[at]["config"]
        branches = entry["branches"]
        if not branches:
            raise ValueError("parallel_branches requires at least one branch")
        vectors, prev = [], None
        for b, bcfg in enumerate(branches):
            xin, min_ = x, mask
            if mutation == "branch_chain" and b == 1:
                xin, min_ = prev
            if mutation == "branch_mask_dropped" and b == len(branches) - 1:
                min_ = None
            y, m = run_layers(xin, min_, bcfg.get("hidden_layers", []), f"rep/{at}/branch{b}", weights, cfg, dtype)
            prev = (y, m)
            keep(b, y, m)
            vectors.append(pool(y, m, bcfg["pooling"], mutation))
        vec = merge(vectors, str(entry.get("merge", "concat")).lower(), mutation)
    logits, _ = of._run_block(vec, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    return {"embedding": vec.detach().numpy(), "prediction": logits.detach().numpy()}


# ---- float32 emulation of the pool-and-merge op's sum order (csrc/jg_poolvec.hip) ------------------------------------------
def emulate_pool(x: np.ndarray, mask: np.ndarray | None, kind: str) -> np.ndarray:
    """One POOLVEC op's pooled vector in float32, in the kernel's order.  x (W, F, L, C) f32, mask (W, F, L) bool or None.
    max / average: 256 / (C / 4) position groups, group g takes positions g, g + groups, ... of the window's F x L in turn,
    the groups are folded in group order, then the sentinel rule or the division.  last: the frames' gathered rows summed in
    frame order, divided by the count of frames."""
    x = np.asarray(x, f32)
    w, f, l, c = x.shape
    if kind == "last":
        out = np.zeros((w, c), f32)
        for i in range(w):
            n = np.full(f, l) if mask is None else mask[i].sum(axis=-1)
            acc = np.zeros(c, f32)
            for r in range(f):
                if n[r] >= 1:
                    acc = (acc + x[i, r, n[r] - 1]).astype(f32)
            div = f32(f) if mask is None else f32(max(int((n >= 1).sum()), 1))
            out[i] = acc / div
        return out
    groups = 256 // (c // 4)
    pos = f * l
    xs = x.reshape(w, pos, c)
    ms = np.ones((w, pos), bool) if mask is None else mask.reshape(w, pos)
    steps = -(-pos // groups)
    padx = np.zeros((w, steps * groups, c), f32)
    padx[:, :pos] = xs
    padm = np.zeros((w, steps * groups), bool)
    padm[:, :pos] = ms
    padx, padm = padx.reshape(w, steps, groups, c), padm.reshape(w, steps, groups)
    is_max = kind == "max"
    acc = np.full((w, groups, c), -np.inf if is_max else 0.0, f32)
    for s in range(steps):
        k = padm[:, s, :, None]
        acc = np.where(k, np.maximum(acc, padx[:, s]) if is_max else (acc + padx[:, s]).astype(f32), acc)
    tot = acc[:, 0]
    for g in range(1, groups):
        tot = np.maximum(tot, acc[:, g]) if is_max else (tot + acc[:, g]).astype(f32)
    cnt = ms.sum(axis=1).astype(f32)[:, None]
    if is_max:
        if mask is None:
            return tot
        return np.where(cnt <= 0, f32(0), np.where(cnt < pos, np.maximum(tot, f32(-1.0e9)), tot)).astype(f32)
    return (tot / (np.maximum(cnt, f32(1e-7)) if mask is not None else f32(pos))).astype(f32)


def emulate_merge(vectors: list, how: str) -> np.ndarray:
    """The merged float32 vector as the ops leave it: store, then add / max in branch order, the last branch of an average
    scaled by float32(1 / n)."""
    if how == "concat":
        return np.concatenate([np.asarray(v, f32) for v in vectors], axis=-1)
    out = np.asarray(vectors[0], f32)
    for v in vectors[1:]:
        out = np.maximum(out, np.asarray(v, f32)) if how == "max" else (out + np.asarray(v, f32)).astype(f32)
    if how == "average":
        out = (out * f32(1.0 / len(vectors))).astype(f32)
    return out
