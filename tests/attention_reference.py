"""Reference side of the frame-attention checks (tests/test_frameattn_reference.py on the CPU, tests/test_gpu_frameattn.py
on the GPU).  Nothing here imports the product: the layer is restated from the reference's source, the model forward
composes it with the functions of ``oracle/forward.py`` as they are.

**The layer** - ``CrossFrameAttention`` (nnlib/v2/layers.py:2283-2384), read, not executed (no TensorFlow here):

* input ``(B, 6, L, C)`` -> ``tf.transpose(inputs, [0, 2, 1, 3])`` -> ``(B * L, 6, C)`` (:2358-2359): at every position the
  six frames are six tokens;
* ``attn_norm = LayerNormalization(epsilon=1e-6)`` (:2321-2323): over C, biased variance, gamma, beta;
* ``mha = MultiHeadAttention(num_heads=H, key_dim=C // H, attention_axes=[1])`` (:2324-2330), called as
  ``mha(x_norm, x_norm)`` (:2363-2365).  Keras: query / key / value ``EinsumDense`` kernels ``(C, H, D)`` + bias ``(H, D)``;
  ``query *= 1 / sqrt(D)`` behind its bias; ``scores = einsum(key, query)``; softmax over the six keys (no mask: the
  outputs of ``tf.transpose`` / ``tf.reshape`` carry none); dropout inert at inference; ``einsum(scores, value)``; output
  ``EinsumDense`` kernel ``(H, D, C)`` + bias ``(C)``;
* ``x = x + attn_out`` (:2367);
* ``use_ffn`` (:2370-2376): ``ffn_norm`` (eps 1e-6, :2335-2337), ``Dense(F, activation="gelu")`` (:2338-2340) - the name
  resolves to ``keras.activations.gelu``, Keras-3 default ``approximate=True``, the tanh form ``oracle/forward.py``
  (``gelu_tanh``) uses for ``activation: gelu`` layers -, ``Dense(C)`` (:2344), ``x = x + ffn_out``;
* back to ``(B, 6, L, C)`` (:2379-2380).  The layer does not set ``supports_masking``: every layer behind it sees no mask.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from oracle import forward as of

LN_EPS = 1e-6
ATTN = "cross_frame_attention"


# ---- the restatement ----------------------------------------------------------------------------------------------------
def layer_norm(x, gamma, beta, eps=LN_EPS, unbiased=False):
    mean = x.mean(axis=-1, keepdims=True)
    d = x - mean
    var = (d * d).sum(axis=-1, keepdims=True) / (x.shape[-1] - (1 if unbiased else 0))
    return d / np.sqrt(var + eps) * gamma + beta


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


def gelu_erf(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x * 0.7071067811865476))


def cross_frame_attention(x, w: dict, heads: int, use_ffn: bool = True, first_half_only: bool = False, mutation: str | None = None):
    """float64.  x (B, 6, L, C); w: the layer's variables by their leaf names (``attn_norm/gamma`` ...
    ``mha/query/kernel`` ... ``ffn_dense2/bias``).  ``mutation``: one of MUTATIONS - a bug a kernel of this layer typically
    has, for the checks that must catch it."""
    x = np.asarray(x, np.float64)
    g = lambda name: np.asarray(w[name], np.float64)
    b_, fr, l, c = x.shape
    d = c // heads
    t = x.transpose(0, 2, 1, 3)                                           # (B, L, 6, C)   :2358
    if mutation == "frames_from_wrong_rows":                              # a reshape where the transpose belongs: token f of
        t = x.reshape(b_, l, fr, c)                                       # position p read from row 6 p + f of the (6 L, C) rows
    ln_kw = dict(eps=1e-3 if mutation == "ln_eps_1e-3" else LN_EPS, unbiased=mutation == "ln_unbiased_variance")
    xn = layer_norm(t, g("attn_norm/gamma"), g("attn_norm/beta"), **ln_kw)      # :2362
    q = np.einsum("blfc,chd->blfhd", xn, g("mha/query/kernel")) + g("mha/query/bias")
    k = np.einsum("blfc,chd->blfhd", xn, g("mha/key/kernel")) + g("mha/key/bias")
    v = np.einsum("blfc,chd->blfhd", xn, g("mha/value/kernel"))
    if mutation != "value_bias_dropped":
        v = v + g("mha/value/bias")
    scale = 1.0 / math.sqrt(d)
    if mutation == "scale_sqrt_channels":
        scale = 1.0 / math.sqrt(c)
    if mutation == "scale_before_bias":
        q = (q - g("mha/query/bias")) * scale + g("mha/query/bias")
    else:
        q = q * scale
    s = np.einsum("blfhd,blghd->blhfg", q, k)                             # (B, L, H, query frame, key frame)
    axis = -2 if mutation == "softmax_over_queries" else -1
    s = s - s.max(axis=axis, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=axis, keepdims=True)
    ctx = np.einsum("blhfg,blghd->blfhd", p, v)
    wo = g("mha/attention_output/kernel")                                 # (H, D, C)
    if mutation == "heads_transposed_in_output_kernel":                   # the kernel read as (D, H, C)
        wo = wo.reshape(d, heads, c).transpose(1, 0, 2)
    out = np.einsum("blfhd,hdc->blfc", ctx, wo) + g("mha/attention_output/bias")
    t = t + out if mutation != "residual_dropped" else out                # :2367
    if use_ffn and not first_half_only:
        xn = layer_norm(t, g("ffn_norm/gamma"), g("ffn_norm/beta"), **ln_kw)     # :2371
        h = xn @ g("ffn_dense1/kernel") + g("ffn_dense1/bias")
        h = gelu_erf(h) if mutation == "erf_gelu" else gelu_tanh(h)
        t = t + (h @ g("ffn_dense2/kernel") + g("ffn_dense2/bias"))       # :2372-2376
    return t.transpose(0, 2, 1, 3)                                        # :2379-2380


MUTATIONS = ("scale_sqrt_channels", "scale_before_bias", "softmax_over_queries", "heads_transposed_in_output_kernel",
             "value_bias_dropped", "erf_gelu", "ln_unbiased_variance", "ln_eps_1e-3", "frames_from_wrong_rows", "residual_dropped")


# ---- weights ------------------------------------------------------------------------------------------------------------
def attention_layers(cfg: dict) -> list[tuple[int, dict]]:
    return [(i, dict(layer.get("config") or {})) for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() == ATTN]


def without_attention(cfg: dict) -> dict:
    """The same model with every attention layer replaced by a dropout layer (the identity at inference, no variables): the
    layers keep their indices - and with them their weight names -, and ``oracle.forward.weight_specs`` understands all of it
    (the attention layer keeps the channel count: embed_dim = incoming channels, builder.py:1165-1166)."""
    out = copy.deepcopy(cfg)
    layers = out["representation_learner"]["hidden_layers"]
    for i, _ in attention_layers(cfg):
        layers[i] = {"name": "dropout", "config": {"rate": 0.0}}
    return out


def layer_specs(c: int, heads: int, ff: int, use_ffn: bool) -> dict[str, tuple]:
    d = c // heads
    s = {"attn_norm/gamma": (c,), "attn_norm/beta": (c,), "mha/attention_output/kernel": (heads, d, c),
         "mha/attention_output/bias": (c,)}
    for part in ("query", "key", "value"):
        s[f"mha/{part}/kernel"] = (c, heads, d)
        s[f"mha/{part}/bias"] = (heads, d)
    if use_ffn:
        s.update({"ffn_norm/gamma": (c,), "ffn_norm/beta": (c,), "ffn_dense1/kernel": (c, ff), "ffn_dense1/bias": (ff,),
                  "ffn_dense2/kernel": (ff, c), "ffn_dense2/bias": (c,)})
    return s


def weight_specs(cfg: dict) -> dict[str, tuple]:
    specs = dict(of.weight_specs(without_attention(cfg)))
    for i, a in attention_layers(cfg):
        for leaf, shp in layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0)),
                                     bool(a.get("use_ffn", True))).items():
            specs[f"rep/{i}/{leaf}"] = shp
    return specs


def random_layer_weights(specs: dict[str, tuple], rng, gain: float = 1.0) -> dict[str, np.ndarray]:
    """Glorot-like kernels (fan-in = the contracted axes), gamma ~ U[0.5, 1.5], beta / bias ~ N(0, 0.1)."""
    out = {}
    for name, shp in sorted(specs.items()):
        leaf = name.rsplit("/", 1)[1]
        if leaf == "kernel":
            fan_in = shp[0] * shp[1] if name.endswith("attention_output/kernel") else shp[0]
            lim = gain * math.sqrt(6.0 / fan_in)
            v = rng.uniform(-lim, lim, shp)
        elif leaf == "gamma":
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.normal(0.0, 0.1, shp)
        out[name] = v.astype(np.float32)
    return out


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    w = dict(of.random_weights(without_attention(cfg), seed))
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for i, a in attention_layers(cfg):
        specs = layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0)), bool(a.get("use_ffn", True)))
        for leaf, v in random_layer_weights(specs, rng).items():
            w[f"rep/{i}/{leaf}"] = v
    return w


def sub_weights(weights: dict, prefix: str) -> dict[str, np.ndarray]:
    n = len(prefix) + 1
    return {k[n:]: v for k, v in weights.items() if k.startswith(prefix + "/")}


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with attention layers: the layers in front of one run through
    ``oracle.forward._run_block`` with the mask they have, the attention through :func:`cross_frame_attention`, the layers
    behind it through ``_run_block`` with ``mask=None`` - masked_batchnorm, the pool (``average`` = the plain mean over all
    6 L positions, layers.py:478-480), a later conv all run unmasked, on the values the graph holds at masked positions.
    A segment is handed to ``_run_block`` with dropout layers in front of it, so that layer i stays layer i (weight names)."""
    idt = torch.as_tensor(np.asarray(ids).astype(np.int64))
    emb_cfg = cfg["embedding"]
    assert emb_cfg.get("use_embedding_layer", False) and not emb_cfg.get("use_positional_embeddings", False)
    table = torch.as_tensor(weights["embedding/embeddings"]).to(dtype)
    x = table[idt]
    mask = (idt != 0).to(dtype)
    rep = cfg["representation_learner"]
    layers = rep["hidden_layers"]
    pad = {"name": "dropout", "config": {}}
    cuts = [i for i, _ in attention_layers(cfg)]
    nmds = []
    start = 0
    for cut in cuts + [len(layers)]:
        last = cut == len(layers)
        seg = [pad] * start + list(layers[start:cut])
        x, n_ = of._run_block(x, mask, seg, "rep", weights, cfg, dtype, pooling=rep.get("pooling") if last else None)
        nmds += n_
        if last:
            break
        a = dict(layers[cut].get("config") or {})
        y = cross_frame_attention(x.detach().numpy(), sub_weights(weights, f"rep/{cut}"), int(a["num_heads"]),
                                  bool(a.get("use_ffn", True)))
        x = torch.as_tensor(y).to(dtype)
        mask = None                                                      # the layer does not set supports_masking
        start = cut + 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- inputs -------------------------------------------------------------------------------------------------------------
def window_ids(l: int, kind: str, n_win: int = 6, seed: int = 11) -> np.ndarray:
    """(n_win, 6, l) codon ids.  ``full``: every codon valid; ``ragged``: windows of different lengths, right-padded with
    id 0, frames 2 / 3 of a strand one codon shorter than frame 1 as the translation leaves them, and N runs inside;
    ``few``: 3 - 12 valid codons per frame, everything else padding."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(1, 65, (n_win, 6, l))
    if kind == "full":
        return ids.astype(np.uint8)
    for w in range(n_win):
        n = int(rng.integers(l // 3, l + 1)) if kind == "ragged" else int(rng.integers(4, 13))
        for f in range(6):
            ids[w, f, max(n - (1 if f % 3 else 0), 0):] = 0
        if kind == "ragged" and w % 2:
            a = int(rng.integers(0, max(n - 6, 1)))
            ids[w, :, a:a + 3] = 0
    assert kind in ("ragged", "few"), kind
    return ids.astype(np.uint8)


# ---- emulation of the kernel's arithmetic (csrc/jg_frameattn.hip), rounding where the kernel rounds -----------------------
f32 = np.float32


def _fma_chain(acc, a, b):
    """acc (T, N) f32 += a (T, K) @ b (K, N), as a k-ordered f32 fma chain (the exact-f32 matrix cores: one rounding per
    product-and-add; the product of two f32 values is exact in f64)."""
    acc = acc.astype(np.float64)
    for k in range(a.shape[1]):
        acc = (acc + a[:, k, None].astype(np.float64) * b[None, k, :].astype(np.float64)).astype(f32).astype(np.float64)
    return acc.astype(f32)


def _ln32(x, eps):
    c = x.shape[-1]
    s = np.zeros(x.shape[:-1], f32)
    for i in range(c):
        s = s + x[..., i]
    mean = s * f32(1.0 / c)
    sq = np.zeros_like(s, dtype=np.float64)
    for i in range(c):
        d = (x[..., i] - mean).astype(np.float64)
        sq = (sq + d * d).astype(f32).astype(np.float64)
    rstd = f32(1.0) / np.sqrt(sq.astype(f32) * f32(1.0 / c) + f32(eps))
    return ((x - mean[..., None]) * rstd[..., None]).astype(f32)


def _gelu32(v):
    t = v * (f32(-2.3022082) - f32(0.10294324) * v * v)
    return (v * (f32(1.0) / (f32(1.0) + np.exp2(t)))).astype(f32)


def fold(w: dict, heads: int, use_ffn: bool) -> dict[str, np.ndarray]:
    """The host-side fold, restated: LN gamma / beta into the kernels and biases behind them, 1 / sqrt(D) into the query;
    float64, rounded to f32 once."""
    g = lambda name: np.asarray(w[name], np.float64)
    c = g("attn_norm/gamma").shape[0]
    d = c // heads
    out = {}
    for part, scale in (("query", 1.0 / math.sqrt(d)), ("key", 1.0), ("value", 1.0)):
        kern = g(f"mha/{part}/kernel").reshape(c, c)
        out[f"w{part[0]}"] = (g("attn_norm/gamma")[:, None] * kern * scale).astype(f32)
        out[f"b{part[0]}"] = ((g("attn_norm/beta") @ kern + g(f"mha/{part}/bias").reshape(c)) * scale).astype(f32)
    out["wo"] = g("mha/attention_output/kernel").reshape(c, c).astype(f32)
    out["bo"] = g("mha/attention_output/bias").astype(f32)
    if use_ffn:
        k1 = g("ffn_dense1/kernel")
        out["w1"] = (g("ffn_norm/gamma")[:, None] * k1).astype(f32)
        out["b1"] = (g("ffn_norm/beta") @ k1 + g("ffn_dense1/bias")).astype(f32)
        out["w2"], out["b2"] = g("ffn_dense2/kernel").astype(f32), g("ffn_dense2/bias").astype(f32)
    return out


def emulate(x, w: dict, heads: int, use_ffn: bool = True) -> np.ndarray:
    """The kernel's arithmetic in numpy: f32 everywhere, one rounding where the kernel has one."""
    x = np.asarray(x, f32)
    b_, fr, l, c = x.shape
    d = c // heads
    fw = fold(w, heads, use_ffn)
    t = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(-1, c)      # tokens (B L 6, C)
    n_tok = t.shape[0]
    xn = _ln32(t, LN_EPS)
    q, k, v = (_fma_chain(np.broadcast_to(fw["b" + p], (n_tok, c)).astype(f32), xn, fw["w" + p]) for p in "qkv")
    q, k, v = (a.reshape(-1, 6, heads, d) for a in (q, k, v))            # (position, frame, head, d)
    s = np.zeros((q.shape[0], heads, 6, 6), np.float64)
    for i in range(d):
        s = (s + q[:, :, None, :, i].transpose(0, 3, 1, 2).astype(np.float64)
             * k[:, None, :, :, i].transpose(0, 3, 1, 2).astype(np.float64)).astype(f32).astype(np.float64)
    s = s.astype(f32)
    e = np.exp2(((s - s.max(axis=-1, keepdims=True)) * f32(1.44269504)).astype(f32)).astype(f32)
    tot = np.zeros(e.shape[:-1], f32)
    for j in range(6):
        tot = tot + e[..., j]
    p = (e * (f32(1.0) / tot)[..., None]).astype(f32)                     # (position, head, query frame, key frame)
    ctx = np.zeros((q.shape[0], 6, heads, d), f32)
    vh = v.transpose(0, 2, 1, 3)                                          # (position, head, key frame, d)
    for i in range(d):
        acc = (p[..., 0] * vh[:, :, 0, i][..., None]).astype(np.float64)
        for j in range(1, 6):
            acc = (acc + p[..., j].astype(np.float64) * vh[:, :, j, i][..., None].astype(np.float64)).astype(f32).astype(np.float64)
        ctx[:, :, :, i] = acc.astype(f32).transpose(0, 2, 1)
    t = _fma_chain((t + fw["bo"]).astype(f32), ctx.reshape(n_tok, c), fw["wo"])
    if use_ffn:
        xn = _ln32(t, LN_EPS)
        h = _gelu32(_fma_chain(np.broadcast_to(fw["b1"], (n_tok, fw["b1"].shape[0])).astype(f32), xn, fw["w1"]))
        t = _fma_chain((t + fw["b2"]).astype(f32), h, fw["w2"])
    return t.reshape(b_, l, 6, c).transpose(0, 2, 1, 3)


# ---- the per-op bound ---------------------------------------------------------------------------------------------------
def errors(got, ref) -> tuple[float, float]:
    """(largest element error, RMS error) of ``got`` against the float64 ``ref``, both in units of the reference's RMS."""
    ref = np.asarray(ref, np.float64)
    d = np.asarray(got, np.float64) - ref
    scale = math.sqrt(float((ref * ref).mean())) or 1.0
    return float(np.abs(d).max()) / scale, math.sqrt(float((d * d).mean())) / scale


def pow2_at_least(v: float) -> float:
    return 2.0 ** math.ceil(math.log2(max(v, 2.0 ** -60)))


HEADROOM = 4.0          # the emulation sits at least this far inside the bound (tests/test_fused_reference.py's margin)
MUTATION_MARGIN = 8.0   # ... and every mutation at least this far outside


def bounds_from(emu, ref) -> dict:
    """The bound of one comparison, set by the emulation's own error on these inputs: the power of two at or above
    HEADROOM x the emulation's element error, and the same for the RMS error."""
    e, r = errors(emu, ref)
    return {"elem": pow2_at_least(HEADROOM * e), "rms": pow2_at_least(HEADROOM * r), "emu_elem": e, "emu_rms": r}


def apply_stages(y, prog, op, dtype=np.float64) -> np.ndarray:
    """The stage list the compiler fused into the op's store (bias / batch norm / activation), with the parameters the
    program's blob holds; in float64 for the reference, in float32 for the emulation."""
    y = np.asarray(y, dtype)
    c = y.shape[-1]
    blob = lambda off: np.asarray(prog.blob[off:off + c], dtype)
    for s in range(op.n_stages):
        st = op.stages[s]
        if st.kind == 1:                                   # JG_ST_BIAS
            y = y + blob(st.p0)
        elif st.kind == 2:                                 # JG_ST_BN: g * ((x - mu) * inv_std) + b
            y = blob(st.p2) * ((y - blob(st.p0)) * blob(st.p1)) + blob(st.p3)
        elif st.kind == 5 and st.arg == 1:                 # JG_ST_ACT, JG_ACT_GELU_TANH
            y = gelu_tanh(y) if dtype == np.float64 else _gelu32(y)
        elif st.kind == 5 and st.arg == 3:
            y = np.maximum(y, dtype(0.0))
        else:
            raise ValueError(f"stage kind {st.kind} arg {st.arg}")
    return y
