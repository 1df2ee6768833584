"""Reference side of the axial-attention checks (tests/test_axialattn_reference.py on the CPU, tests/test_gpu_axialattn.py
on the GPU).  Nothing here imports the product: the layers are restated from the reference's source, the model forward
composes them with the functions of ``oracle/forward.py`` as they are.

**The length half** - ``TransformerEncoder`` (nnlib/v2/layers.py:2206-2280) with ``attention_axes = 2``, read, not executed
(no TensorFlow here):

* ``x_norm = attn_norm(inputs)``, ``LayerNormalization(epsilon=1e-6)`` (:2224-2226, :2249);
* ``mha(x_norm, x_norm)`` (:2252-2254), ``MultiHeadAttention(H, key_dim = C // H, attention_axes=[2])``: on ``(B, 6, L, C)``
  the attention runs over the L positions inside every (batch, frame) row.  No ``attention_mask`` is passed; Keras 3
  (the reference pins ``keras >= 3.12``) fills ``query_mask`` / ``value_mask`` of ``MultiHeadAttention.call`` from the
  ``_keras_mask`` of its tensor arguments, and ``LayerNormalization`` passes its input's mask on.  With the implicit mask
  ``m`` the layer attends under ``M[q, k] = m[q] and m[k]``: masked scores get -1e9 added, and Keras' masked softmax
  multiplies the probabilities by ``M`` afterwards.  So: a VALID query takes its softmax over the valid keys (a masked
  key's exp is exactly 0; the query is its own valid key); a MASKED query's probabilities are all multiplied by 0 - its
  context is exactly zero, its attention output the output projection's bias alone;
* ``x = inputs + attn_out`` (:2256); ``ffn_norm`` (eps 1e-6), ``Dense(F, activation="gelu")`` (the tanh form, as in
  tests/attention_reference.py), ``Dense(C)``, ``x + ffn_out`` (:2259-2264) - at every position, masked ones included;
* the layer does not set ``supports_masking``: behind a stand-alone ``transformer_encoder`` nothing sees a mask.

**The layer** - ``AxialAttention`` (:2400-2517): per block ``r = x; x = length_attn(x); x = frame_attn(x); x = norm(x);
x += r`` (:2485-2501).  Only a tensor that leaves a layer carries ``_keras_mask``: block 0's encoder sees the layer's
incoming mask, from block 1 on ``x`` is the result of ``+=`` inside ``call`` and carries none.  ``frame_attn`` is
``CrossFrameAttention(use_ffn=True)`` (tests/attention_reference.py), unmasked.  The post norm (:2448-2457, :2493-2498):
``layernorm`` = Keras ``LayerNormalization(epsilon)``, unmasked; ``masked_layernorm`` / ``masked_dyt`` are called with the
layer's incoming mask, in every block; ``masked_batchnorm`` is called without one (the inference affine).  The layer sets
``supports_masking`` (:2442) and does not override ``compute_mask``: the mask survives it.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import attention_reference as ar
import local_attention_reference as lr
from attention_reference import f32, gelu_tanh, layer_norm
from oracle import forward as of

LN_EPS = 1e-6
AXIAL, ENCODER = "axial_attention", "transformer_encoder"
NORM_TYPES = ("layernorm", "masked_layernorm", "masked_dyt", "masked_batchnorm")


# ---- the restatement ----------------------------------------------------------------------------------------------------
def transformer_encoder(x, w: dict, heads: int, mask=None, mutation: str | None = None, eps: float = LN_EPS):
    """float64.  x (R, L, C) frame rows; mask (R, L) validity of queries and keys, or None (all valid); w: the layer's
    variables by their leaf names (``attn_norm/gamma`` ... ``mha/query/kernel`` ... ``ffn_dense2/bias``).  ``eps``: of the
    two layer norms (1e-6 in the reference; the mutation that takes the post norm's passes another)."""
    x = np.asarray(x, np.float64)
    g = lambda name: np.asarray(w[name], np.float64)
    r_, l, c = x.shape
    d = c // heads
    valid = np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool)
    key_ok = np.ones((r_, l), bool) if mutation == "key_mask_ignored" else valid
    xn = layer_norm(x, g("attn_norm/gamma"), g("attn_norm/beta"), eps=eps)
    proj = lambda part: (xn @ g(f"mha/{part}/kernel").reshape(c, c)).reshape(r_, l, heads, d) + g(f"mha/{part}/bias")
    q, k, v = proj("query"), proj("key"), proj("value")                  # (R, L, H, D)
    q = q * (1.0 / math.sqrt(c if mutation == "scale_sqrt_channels" else d))
    s = q.transpose(0, 2, 1, 3) @ k.transpose(0, 2, 3, 1)                # (R, H, query, key)
    if mutation == "softmax_over_queries":
        m = np.broadcast_to(valid[:, None, :, None], s.shape)              # (the queries a key's column is normalised over)
        s = np.where(m, s, -np.inf)
        mx = s.max(axis=-2, keepdims=True)
        e = np.where(m, np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
        tot = e.sum(axis=-2, keepdims=True)
        p = e / np.where(tot > 0, tot, 1.0) * key_ok[:, None, None, :]
    else:
        m = np.broadcast_to(key_ok[:, None, None, :], s.shape)
        s = np.where(m, s, -np.inf)
        mx = s.max(axis=-1, keepdims=True)
        e = np.where(m, np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
        tot = e.sum(axis=-1, keepdims=True)
        p = e / np.where(tot > 0, tot, 1.0)
    ctx = (p @ v.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)            # (R, L, H, D)
    if mutation == "masked_query_uniform":                                 # a softmax over -1e9 everywhere, not multiplied by M
        ctx = np.where(valid[:, :, None, None], ctx, v.mean(axis=1, keepdims=True))
    elif mutation != "query_mask_ignored":
        ctx = np.where(valid[:, :, None, None], ctx, 0.0)
    out = ctx.reshape(r_, l, c) @ g("mha/attention_output/kernel").reshape(c, c)
    bias = g("mha/attention_output/bias")
    if mutation == "bias_dropped_at_masked_queries":
        out = out + np.where(valid[:, :, None], bias, 0.0)
    else:
        out = out + bias
    t = x + out
    xn = layer_norm(t, g("ffn_norm/gamma"), g("ffn_norm/beta"), eps=eps)
    h = gelu_tanh(xn @ g("ffn_dense1/kernel") + g("ffn_dense1/bias"))
    return t + (h @ g("ffn_dense2/kernel") + g("ffn_dense2/bias"))


def post_norm(x, w: dict, norm_type: str, epsilon: float, mask=None, mutation: str | None = None):
    """float64, x (B, 6, L, C), mask (B, 6, L) bool or None: the norm that closes a block."""
    g = lambda name: np.asarray(w[name], np.float64)
    mk = None if mask is None else np.asarray(mask, np.float64)[..., None]
    if norm_type == "layernorm":
        if mutation == "post_norm_masked_under_layernorm" and mk is not None:
            return layer_norm(x * mk, g("gamma"), g("beta"), eps=epsilon) * mk
        return layer_norm(x, g("gamma"), g("beta"), eps=epsilon)
    if norm_type == "masked_layernorm":                                    # layers.py:335-367
        if mk is None:
            return layer_norm(x, g("gamma"), g("beta"), eps=epsilon)
        return layer_norm(x * mk, g("gamma"), g("beta"), eps=epsilon) * mk
    if norm_type == "masked_dyt":                                          # layers.py:431-444
        y = np.tanh(g("alpha") * x) * g("gamma") + g("beta")
        return y if mk is None else y * mk
    if norm_type == "masked_batchnorm":                                    # layers.py:918-938, inference, no mask
        return g("gamma") * ((x - g("moving_mean")) / np.sqrt(g("moving_variance") + epsilon)) + g("beta")
    raise ValueError(f"Unsupported norm_type: {norm_type}")


def axial_attention(x, w: dict, heads: int, blocks: int = 1, norm_type: str = "layernorm", epsilon: float = 1e-6,
                    mask=None, mutation: str | None = None):
    """float64.  x (B, 6, L, C), mask (B, 6, L) or None; w: ``block<j>/length/<leaf>``, ``block<j>/frame/<leaf>``,
    ``block<j>/post_norm/<var>``."""
    x = np.asarray(x, np.float64)
    b_, fr, l, c = x.shape
    mk = None if mask is None else np.asarray(mask).reshape(b_, fr, l) != 0
    enc_mut = mutation if mutation in ENCODER_MUTATIONS else None
    for j in range(blocks):
        wl, wf, wn = (ar.sub_weights(w, f"block{j}/{part}") for part in ("length", "frame", "post_norm"))
        r = x
        m_j = mk if (j == 0 or mutation == "mask_in_block1_as_well") else None
        length = lambda t: transformer_encoder(t.reshape(b_ * fr, l, c), wl, heads, None if m_j is None else m_j.reshape(b_ * fr, l),
                                               enc_mut, eps=epsilon if mutation == "post_norm_epsilon_in_inner_norms" else LN_EPS
                                               ).reshape(b_, fr, l, c)
        frame = lambda t: ar.cross_frame_attention(t, wf, heads, True)
        if mutation == "frame_half_before_length_half":
            x = length(frame(x))
        else:
            x = length(x)
            if mutation == "residual_taken_after_length_half":
                r = x
            x = frame(x)
        x = post_norm(x, wn, norm_type, epsilon, mk, mutation) + r
    return x


ENCODER_MUTATIONS = ("key_mask_ignored", "query_mask_ignored", "masked_query_uniform", "softmax_over_queries",
                     "scale_sqrt_channels", "bias_dropped_at_masked_queries")
MUTATIONS = ENCODER_MUTATIONS + ("mask_in_block1_as_well", "post_norm_epsilon_in_inner_norms", "post_norm_masked_under_layernorm",
                                 "residual_taken_after_length_half", "frame_half_before_length_half")

KINDS = ("full", "ragged", "few", "long_n", "empty_fwd")

#: the input kinds on which a mutation must show.  The mask mutations need masked positions: on ``full`` every position is
#: valid and they change nothing, by construction.  ``softmax_over_queries`` shows on every kind with more than one key.
#: ``post_norm_epsilon_in_inner_norms`` needs a layer whose epsilon is not the encoders' 1e-6 (the mutation check runs at
#: 1e-3), ``mask_in_block1_as_well`` two blocks (it runs with two).
_MASKED = ("ragged", "few", "long_n", "empty_fwd")
VISIBLE_ON = {
    "key_mask_ignored": _MASKED,
    "query_mask_ignored": _MASKED,
    "masked_query_uniform": _MASKED,
    "softmax_over_queries": KINDS,
    "scale_sqrt_channels": KINDS,
    "bias_dropped_at_masked_queries": _MASKED,
    "mask_in_block1_as_well": _MASKED,
    "post_norm_epsilon_in_inner_norms": KINDS,
    "post_norm_masked_under_layernorm": _MASKED,
    "residual_taken_after_length_half": KINDS,
    "frame_half_before_length_half": KINDS,
}


# ---- weights ------------------------------------------------------------------------------------------------------------
def attention_layers(cfg: dict) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {}))
            for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() in (AXIAL, ENCODER, ar.ATTN)]


def without_attention(cfg: dict) -> dict:
    out = copy.deepcopy(cfg)
    for i, _, _ in attention_layers(cfg):
        out["representation_learner"]["hidden_layers"][i] = {"name": "dropout", "config": {"rate": 0.0}}
    return out


def norm_type_of(a: dict) -> str:
    nt = str(a.get("norm_type", "layernorm")).lower()
    return "layernorm" if nt == "layer_normalization" else nt


def norm_specs(norm_type: str, c: int) -> dict[str, tuple]:
    return dict(of._norm_vars("masked_layernorm" if norm_type == "layernorm" else norm_type, c))


def encoder_specs(c: int, heads: int, ff: int) -> dict[str, tuple]:
    return ar.layer_specs(c, heads, ff, True)


def layer_specs(c: int, heads: int, ff: int, blocks: int, norm_type: str) -> dict[str, tuple]:
    s = {}
    for j in range(blocks):
        for part in ("length", "frame"):
            s.update({f"block{j}/{part}/{leaf}": shp for leaf, shp in encoder_specs(c, heads, ff).items()})
        s.update({f"block{j}/post_norm/{leaf}": shp for leaf, shp in norm_specs(norm_type, c).items()})
    return s


def _specs_of(kind: str, a: dict) -> dict[str, tuple]:
    c, h, f = int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0))
    if kind == AXIAL:
        return layer_specs(c, h, f, int(a.get("num_blocks", 1)), norm_type_of(a))
    if kind == ENCODER:
        return encoder_specs(c, h, f)
    return ar.layer_specs(c, h, f, bool(a.get("use_ffn", True)))


def weight_specs(cfg: dict) -> dict[str, tuple]:
    specs = dict(of.weight_specs(without_attention(cfg)))
    for i, kind, a in attention_layers(cfg):
        for leaf, shp in _specs_of(kind, a).items():
            specs[f"rep/{i}/{leaf}"] = shp
    return specs


def random_layer_weights(specs: dict[str, tuple], rng) -> dict[str, np.ndarray]:
    """``attention_reference.random_layer_weights`` plus the batch norm's / DyT's variables."""
    out = ar.random_layer_weights(specs, rng)
    for name, shp in sorted(specs.items()):
        leaf = name.rsplit("/", 1)[1]
        if leaf == "moving_variance":
            out[name] = rng.uniform(0.5, 1.5, shp).astype(np.float32)
        elif leaf == "alpha":
            out[name] = np.full(shp, 0.5, np.float32)
    return out


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    w = dict(of.random_weights(without_attention(cfg), seed))
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for i, kind, a in attention_layers(cfg):
        for leaf, v in random_layer_weights(_specs_of(kind, a), rng).items():
            w[f"rep/{i}/{leaf}"] = v
    return w


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with attention layers, composed as ``attention_reference.forward`` does it.
    Behind a ``cross_frame_attention`` or a ``transformer_encoder`` no mask exists; behind an ``axial_attention`` the mask
    is kept."""
    idt = torch.as_tensor(np.asarray(ids).astype(np.int64))
    emb_cfg = cfg["embedding"]
    assert emb_cfg.get("use_embedding_layer", False) and not emb_cfg.get("use_positional_embeddings", False)
    table = torch.as_tensor(weights["embedding/embeddings"]).to(dtype)
    x = table[idt]
    mask = (idt != 0).to(dtype)
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    pad = {"name": "dropout", "config": {}}
    nmds = []
    start = 0
    for cut, kind, a in attention_layers(cfg) + [(len(layers), "", {})]:
        last = cut == len(layers)
        seg = [pad] * start + list(layers[start:cut])
        x, n_ = of._run_block(x, mask, seg, "rep", weights, cfg, dtype, pooling=rep.get("pooling") if last else None)
        nmds += n_
        if last:
            break
        mask = lr._mask_behind(mask, seg, cfg, dtype)
        lw = ar.sub_weights(weights, f"rep/{cut}")
        xin = x.detach().numpy()
        mk = None if mask is None else mask.numpy() != 0
        if kind == ar.ATTN:
            y = ar.cross_frame_attention(xin, lw, int(a["num_heads"]), bool(a.get("use_ffn", True)))
            mask = None
        elif kind == ENCODER:
            b_, fr, l, c = xin.shape
            y = transformer_encoder(xin.reshape(b_ * fr, l, c), lw, int(a["num_heads"]),
                                    None if mk is None else mk.reshape(b_ * fr, l)).reshape(b_, fr, l, c)
            mask = None                                                  # the layer does not set supports_masking
        else:
            y = axial_attention(xin, lw, int(a["num_heads"]), int(a.get("num_blocks", 1)), norm_type_of(a),
                                float(a.get("epsilon", 1e-6)), mk)
        x = torch.as_tensor(y).to(dtype)
        start = cut + 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- inputs -------------------------------------------------------------------------------------------------------------
def window_ids(l: int, kind: str, n_win: int = 5, seed: int = 17, chunk: int = 64, grow: int = 0) -> np.ndarray:
    """(n_win, 6, l) codon ids.  ``full`` / ``ragged`` / ``few``: tests/attention_reference.py.  ``long_n``: one run of
    invalid codons longer than ``chunk`` (+ ``grow``: by how much the convs in front shorten it) in every other row, as long
    as the row allows.  ``empty_fwd``: ragged windows, and the three forward frames of window 1 hold no valid codon at all
    (whole rows masked: every query of them is a masked query, no key of them valid)."""
    if kind in ("full", "ragged", "few"):
        return ar.window_ids(l, kind, n_win, seed)
    if kind == "long_n":
        return lr.window_ids(l, "long_n", n_win=n_win, seed=seed, half=(chunk + 1) // 2, grow=grow)
    assert kind == "empty_fwd", kind
    ids = ar.window_ids(l, "ragged", n_win, seed)
    ids[min(1, n_win - 1), :3, :] = 0
    return ids


value_inputs = lr.value_inputs


# ---- emulation of the kernel's arithmetic (csrc/jg_lengthattn.hip), rounding where the kernel rounds ----------------------
STEP = 16                # keys per update of the kernel's online softmax (JG_LENGTHATTN_STEP); chunks of 64 hold four steps


def fold(w: dict, heads: int) -> dict[str, np.ndarray]:
    """The host-side fold of one encoder, restated (``attention_reference.fold``: the same leaf names)."""
    return ar.fold(w, heads, True)


blob_of = lr.blob_of


def evaluate_fold(x, fw: dict, heads: int, mask=None):
    """The folded operands evaluated plainly in float64 - what the kernel computes, in exact arithmetic."""
    x = np.asarray(x, np.float64)
    r_, l, c = x.shape
    d = c // heads
    g = lambda k: np.asarray(fw[k], np.float64)
    valid = np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool)
    ones, zeros = np.ones(c), np.zeros(c)
    xn = layer_norm(x, ones, zeros)
    q, k, v = ((xn @ g("w" + p) + g("b" + p)).reshape(r_, l, heads, d) for p in "qkv")
    m = valid[:, None, None, :]
    s = np.where(m, np.einsum("rqhd,rkhd->rhqk", q, k), -np.inf)
    mx = s.max(axis=-1, keepdims=True)
    e = np.where(m, np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
    tot = e.sum(axis=-1, keepdims=True)
    ctx = np.einsum("rhqk,rkhd->rqhd", e / np.where(tot > 0, tot, 1.0), v)
    ctx = np.where(valid[:, :, None, None], ctx, 0.0).reshape(r_, l, c)
    t = x + ctx @ g("wo") + g("bo")
    return t + gelu_tanh(layer_norm(t, ones, zeros) @ g("w1") + g("b1")) @ g("w2") + g("b2")


def _r32(a):
    return np.asarray(a, np.float64).astype(f32).astype(np.float64)


def emulate_encoder(x, w: dict, heads: int, mask=None, step: int = STEP) -> np.ndarray:
    """The kernel's arithmetic in numpy: f32 everywhere, one rounding where the kernel has one; the online softmax
    advances ``step`` keys at a time with a running maximum and sum per (query, head), an invalid key's score selected to
    -inf and its v row zeroed, a masked query's context forced to zero.  x (R, L, C)."""
    x = np.asarray(x, f32)
    r_, l, c = x.shape
    d = c // heads
    fw = fold(w, heads)
    valid = np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool)
    t = x.reshape(-1, c)
    n_tok = t.shape[0]
    xn = ar._ln32(t, LN_EPS)
    q, k, v = (ar._fma_chain(np.broadcast_to(fw["b" + p], (n_tok, c)).astype(f32), xn, fw["w" + p]).reshape(r_, l, heads, d) for p in "qkv")
    v = np.where(valid[:, :, None, None], v, f32(0.0)).astype(f32)
    q64 = q.astype(np.float64)
    log2e = np.float64(f32(1.44269504))
    m_run = np.full((r_, l, heads), -np.inf)                              # (f32 values held in float64 arrays)
    l_run = np.zeros((r_, l, heads))
    o = np.zeros((r_, l, heads, d))
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, l, step):
            kk, vv, ok = k[:, t0:t0 + step].astype(np.float64), v[:, t0:t0 + step].astype(np.float64), valid[:, t0:t0 + step]
            n = kk.shape[1]
            s = np.zeros((r_, l, heads, n))
            for i in range(d):                                            # k-ordered fma chain over the head's channels
                s = _r32(s + q64[:, :, None, :, i].transpose(0, 1, 3, 2) * kk[:, None, :, :, i].transpose(0, 1, 3, 2))
            s = np.where(ok[:, None, None, :], s, -np.inf)
            mx = np.maximum(m_run, s.max(axis=-1))
            msafe = np.where(np.isfinite(mx), mx, 0.0)
            scale = _r32(np.exp2(_r32(_r32(m_run - msafe) * log2e).astype(f32)))
            p = _r32(np.exp2(_r32(_r32(s - msafe[..., None]) * log2e).astype(f32)))
            lsum = np.zeros((r_, l, heads))
            for j in range(n):
                lsum = _r32(lsum + p[..., j])
            l_run = _r32(l_run * scale + lsum)                            # (one fma)
            acc = _r32(o * scale[..., None])
            for j in range(n):
                acc = _r32(acc + p[..., j, None] * vv[:, None, j])
            o = acc
            m_run = mx
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(l_run > 0, _r32(1.0 / l_run), 0.0)
    ctx = _r32(o * inv[..., None])
    ctx = np.where(valid[:, :, None, None], ctx, 0.0).astype(f32)
    t = ar._fma_chain((t + fw["bo"]).astype(f32), ctx.reshape(n_tok, c), fw["wo"])
    xn = ar._ln32(t, LN_EPS)
    h = ar._gelu32(ar._fma_chain(np.broadcast_to(fw["b1"], (n_tok, fw["b1"].shape[0])).astype(f32), xn, fw["w1"]))
    return ar._fma_chain((t + fw["b2"]).astype(f32), h, fw["w2"]).reshape(r_, l, c)


def _post_norm32(x, w: dict, norm_type: str, epsilon: float, mask):
    """The element-wise op that closes a block, in f32 (its arithmetic is the engine's older kernels': not restated to the
    rounding - the f32 evaluation of the float64 formula)."""
    return post_norm(np.asarray(x, f32).astype(np.float64), {k: np.asarray(v, f32) for k, v in w.items()}, norm_type, epsilon, mask).astype(f32)


def emulate(x, w: dict, heads: int, blocks: int = 1, norm_type: str = "layernorm", epsilon: float = 1e-6, mask=None) -> np.ndarray:
    """The emulated layer on x (B, 6, L, C): the length half emulated to the rounding, the frame half by
    ``attention_reference.emulate``, the post norm and the add in f32."""
    x = np.asarray(x, f32)
    b_, fr, l, c = x.shape
    mk = None if mask is None else np.asarray(mask).reshape(b_, fr, l) != 0
    for j in range(blocks):
        wl, wf, wn = (ar.sub_weights(w, f"block{j}/{part}") for part in ("length", "frame", "post_norm"))
        r = x
        m_j = mk if j == 0 else None
        t = emulate_encoder(x.reshape(b_ * fr, l, c), wl, heads, None if m_j is None else m_j.reshape(b_ * fr, l)).reshape(b_, fr, l, c)
        t = ar.emulate(t, wf, heads, True)
        x = (_post_norm32(t, wn, norm_type, epsilon, mk) + r).astype(f32)
    return x


# ---- the per-op bound, over ALL positions -------------------------------------------------------------------------------
errors = ar.errors
bounds_from = ar.bounds_from
HEADROOM, MUTATION_MARGIN = ar.HEADROOM, ar.MUTATION_MARGIN


# ---- the fixture model ----------------------------------------------------------------------------------------------------
FIXTURE = dict(embed_dim=32, num_heads=4, feed_forward_dim=128, dropout_rate=0.1, num_blocks=1)
