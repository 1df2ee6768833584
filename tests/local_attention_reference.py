"""Reference side of the local-attention checks (tests/test_localattn_reference.py on the CPU, tests/test_gpu_localattn.py
on the GPU).  Nothing here imports the product: the layer is restated from the reference's source, the model forward
composes it with the functions of ``oracle/forward.py`` as they are.

**The layer** - ``LocalAttention`` (nnlib/v2/layers.py:2520-2645), read, not executed (no TensorFlow here):

* input ``(B, 6, L, C)`` -> ``tf.reshape`` -> ``(B * 6, L, C)`` (:2600): inside every frame row the positions are tokens.
  A reshaped tensor carries no implicit Keras mask: the only mask MultiHeadAttention sees is the explicit one;
* ``attn_mask[q, k] = |q - k| <= window_size // 2`` (:2579-2585), ANDed with the key validity ``mask[r, k]`` when a mask
  arrives (:2604-2609); the same mask serves every block;
* per block (:2611-2623): ``ln1 = LayerNormalization(epsilon=1e-6)``; ``mha = MultiHeadAttention(H, key_dim = C // H)``
  called as ``mha(x_norm, x_norm, attention_mask=attn_mask)`` - query / key / value ``EinsumDense`` kernels ``(C, H, D)`` +
  bias ``(H, D)``, ``query *= 1 / sqrt(D)`` behind its bias, masked scores get -1e9 added, softmax over the keys, output
  ``EinsumDense`` ``(H, D, C)`` + bias ``(C)``; ``x = x + attn``; ``ln2`` (eps 1e-6), ``Dense(F, activation="gelu")`` (the
  tanh form, as in tests/attention_reference.py), ``Dense(C)``, ``x = x + ffn``.  The feed-forward half is always there;
* ``compute_mask`` returns the mask (:2627-2628), ``supports_masking = True`` (:2550): the layers behind see the mask.

**Dead positions.**  A query whose band holds no valid key has no defined value: with -1e9 added to every score of the row
Keras' float32 softmax turns uniform over all L keys, a float64 one does not, newer Keras zeroes such rows.  The restatement
marks them (``dead``) and writes zeros there, as the engine's op does; comparisons run over the live positions.  Dead
positions are masked (a valid position is its own key), so nothing valid depends on them as long as every later reader
masks - the model forward below puts a large value there to show exactly that.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import attention_reference as ar
from attention_reference import f32, gelu_erf, gelu_tanh, layer_norm
from oracle import forward as of

LN_EPS = 1e-6
LOCAL = "local_attention"
DEAD_FILL = 1.0e3       # what the model forward holds at dead positions (any finite value: no valid output may see it)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def attention_mask(l: int, window: int, mask, mutation: str | None = None) -> np.ndarray:
    """(R, L, L) bool: M[r, q, k] = (|q - k| <= window // 2) and mask[r, k]  (mask None: the band alone, R = 1)."""
    half = (window - 1) // 2 if mutation == "half_window_(w-1)//2" else window // 2
    q, k = np.arange(l)[:, None], np.arange(l)[None, :]
    band = np.abs(q - k) < half if mutation == "band_strict" else np.abs(q - k) <= half
    if mutation == "causal_band":
        band = band & (k <= q)
    m = band[None]
    if mask is not None and mutation != "key_mask_ignored":
        mk = np.asarray(mask, bool)
        m = m & (mk[:, :, None] if mutation == "query_mask_for_key_mask" else mk[:, None, :])
    return m


def local_attention_block(x, w: dict, heads: int, window: int, mask=None, mutation: str | None = None):
    """float64, one block.  x (R, L, C) frame rows; mask (R, L) key validity or None; w: the block's variables by their
    leaf names (``ln1/gamma`` ... ``mha/query/kernel`` ... ``ffn2/bias``).  Returns (y, dead): y (R, L, C) with zeros at
    dead positions, dead (R, L) bool.  ``mutation``: one of MUTATIONS."""
    x = np.asarray(x, np.float64)
    g = lambda name: np.asarray(w[name], np.float64)
    r_, l, c = x.shape
    d = c // heads
    half = window // 2
    m = np.broadcast_to(attention_mask(l, window, mask, mutation), (r_, l, l))
    true_m = np.broadcast_to(attention_mask(l, window, mask), (r_, l, l))
    dead = ~true_m.any(axis=-1)
    xn = layer_norm(x, g("ln1/gamma"), g("ln1/beta"))
    q = np.einsum("rlc,chd->rlhd", xn, g("mha/query/kernel")) + g("mha/query/bias")
    k = np.einsum("rlc,chd->rlhd", xn, g("mha/key/kernel")) + g("mha/key/bias")
    v = np.einsum("rlc,chd->rlhd", xn, g("mha/value/kernel"))
    if mutation != "value_bias_dropped":
        v = v + g("mha/value/bias")
    q = q * (1.0 / math.sqrt(c if mutation == "scale_sqrt_channels" else d))
    if mutation in ("halo_from_adjacent_row", "keys_beyond_L"):
        # the band runs over the row's ends: into the neighbouring rows' tokens as they lie in memory (row r's tail and row
        # r + 1's head are adjacent), or onto zero-filled tokens (x = 0: LN gives 0, k / v are their biases) taken as keys
        if mutation == "halo_from_adjacent_row":
            flat = lambda a: np.concatenate([np.zeros((half,) + a.shape[2:]), a.reshape((-1,) + a.shape[2:]), np.zeros((half,) + a.shape[2:])])
            kf, vf = flat(k), flat(v)
            okf = np.concatenate([np.zeros(half, bool), (np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool)).ravel(), np.zeros(half, bool)])
            pick = lambda a, r: a[r * l:r * l + l + 2 * half]
        else:
            zero_tok = lambda bias_name, kern: np.einsum("c,chd->hd", g("ln1/beta"), g(kern)) + g(bias_name)
            padrow = lambda a, tok: np.concatenate([np.broadcast_to(tok, (r_, half) + tok.shape), a, np.broadcast_to(tok, (r_, half) + tok.shape)], axis=1)
            kp, vp = padrow(k, zero_tok("mha/key/bias", "mha/key/kernel")), padrow(v, zero_tok("mha/value/bias", "mha/value/kernel"))
            okp = np.concatenate([np.ones((r_, half), bool), np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool),
                                  np.ones((r_, half), bool)], axis=1)
            pick = None
        ctx = np.zeros((r_, l, heads, d))
        for r in range(r_):
            kk, vv, ok = (pick(kf, r), pick(vf, r), pick(okf, r)) if pick else (kp[r], vp[r], okp[r])
            qq, kq = np.arange(l)[:, None], np.arange(l + 2 * half)[None, :] - half
            mm = (np.abs(qq - kq) <= half) & ok[None, :]
            s = np.einsum("qhd,khd->hqk", q[r], kk)
            s = np.where(mm[None], s, -np.inf)
            mx = s.max(axis=-1, keepdims=True)
            p = np.where(mm[None], np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
            tot = p.sum(axis=-1, keepdims=True)
            p = p / np.where(tot > 0, tot, 1.0)
            ctx[r] = np.einsum("hqk,khd->qhd", p, vv)
    else:
        s = np.einsum("rqhd,rkhd->rhqk", q, k)
        s = np.where(m[:, None], s, -np.inf)
        mx = s.max(axis=-1, keepdims=True)
        e = np.where(m[:, None], np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
        if mutation == "denominator_over_masked_keys":                     # the band's masked keys counted in the sum
            band = np.broadcast_to(attention_mask(l, window, None), (r_, l, l))
            s_all = np.einsum("rqhd,rkhd->rhqk", q, k)
            tot = np.where(band[:, None], np.exp(s_all - np.where(np.isfinite(mx), mx, 0.0)), 0.0).sum(axis=-1, keepdims=True)
        else:
            tot = e.sum(axis=-1, keepdims=True)
        p = e / np.where(tot > 0, tot, 1.0)
        ctx = np.einsum("rhqk,rkhd->rqhd", p, v)
    out = np.einsum("rlhd,hdc->rlc", ctx, g("mha/attention_output/kernel")) + g("mha/attention_output/bias")
    t = x + out
    xn = layer_norm(t, g("ln2/gamma"), g("ln2/beta"))
    h = xn @ g("ffn1/kernel") + g("ffn1/bias")
    h = gelu_erf(h) if mutation == "erf_gelu" else gelu_tanh(h)
    t = t + (h @ g("ffn2/kernel") + g("ffn2/bias"))
    t[dead] = 0.0
    return t, dead


def local_attention(x, w: dict, heads: int, window: int, blocks: int, mask=None, mutation: str | None = None):
    """The layer: ``blocks`` blocks on x (B, 6, L, C) with mask (B, 6, L) or None; w: ``block<j>/<leaf>``.  Returns
    (y (B, 6, L, C), dead (B, 6, L))."""
    x = np.asarray(x, np.float64)
    b_, fr, l, c = x.shape
    t = x.reshape(b_ * fr, l, c)
    mk = None if mask is None else np.asarray(mask).reshape(b_ * fr, l) != 0
    dead = np.zeros((b_ * fr, l), bool)
    for j in range(blocks):
        src = 0 if (mutation == "block2_uses_block1_value_kernel" and j > 0) else j
        wb = ar.sub_weights(w, f"block{j}")
        if src != j:
            wb["mha/value/kernel"] = w["block0/mha/value/kernel"]
        t, dead = local_attention_block(t, wb, heads, window, mk, None if mutation == "block2_uses_block1_value_kernel" else mutation)
    return t.reshape(b_, fr, l, c), dead.reshape(b_, fr, l)


MUTATIONS = ("band_strict", "half_window_(w-1)//2", "causal_band", "key_mask_ignored", "query_mask_for_key_mask",
             "halo_from_adjacent_row", "keys_beyond_L", "denominator_over_masked_keys", "block2_uses_block1_value_kernel",
             "scale_sqrt_channels", "value_bias_dropped", "erf_gelu")

KINDS = ("full", "ragged", "few", "long_n", "short_n")

#: the input kinds on which a mutation must show; on the others it is reported as invisible or as a bonus.  The mask
#: mutations need masked keys inside a live query's band (not ``full``); the row-end mutations need valid keys at a row's
#: ends (``full``; on the other kinds the neighbouring row's tail is padding).  ``half_window_(w-1)//2`` shows for even
#: window sizes only (the tests use 16).  ``few`` holds 3 - 12 valid codons a row: with half-window 8 nearly every band
#: covers them all, so the band mutations are not required there.
VISIBLE_ON = {
    "band_strict": ("full", "ragged", "long_n", "short_n"),
    "half_window_(w-1)//2": ("full", "ragged", "long_n", "short_n"),
    "causal_band": KINDS,
    "key_mask_ignored": ("ragged", "few", "long_n", "short_n"),
    "query_mask_for_key_mask": ("ragged", "few", "long_n", "short_n"),
    "halo_from_adjacent_row": ("full",),
    "keys_beyond_L": ("full",),
    "denominator_over_masked_keys": ("ragged", "few", "long_n", "short_n"),
    "block2_uses_block1_value_kernel": KINDS,
    "scale_sqrt_channels": KINDS,
    "value_bias_dropped": KINDS,
    "erf_gelu": KINDS,
}


# ---- weights ------------------------------------------------------------------------------------------------------------
def attention_layers(cfg: dict) -> list[tuple[int, str, dict]]:
    return [(i, str(layer.get("name", "")).lower(), dict(layer.get("config") or {}))
            for i, layer in enumerate(cfg["representation_learner"]["hidden_layers"])
            if str(layer.get("name", "")).lower() in (LOCAL, ar.ATTN)]


def without_attention(cfg: dict) -> dict:
    """The same model with every attention layer replaced by a dropout layer (see tests/attention_reference.py)."""
    out = copy.deepcopy(cfg)
    for i, _, _ in attention_layers(cfg):
        out["representation_learner"]["hidden_layers"][i] = {"name": "dropout", "config": {"rate": 0.0}}
    return out


def block_specs(c: int, heads: int, ff: int) -> dict[str, tuple]:
    d = c // heads
    s = {"ln1/gamma": (c,), "ln1/beta": (c,), "mha/attention_output/kernel": (heads, d, c), "mha/attention_output/bias": (c,),
         "ln2/gamma": (c,), "ln2/beta": (c,), "ffn1/kernel": (c, ff), "ffn1/bias": (ff,), "ffn2/kernel": (ff, c), "ffn2/bias": (c,)}
    for part in ("query", "key", "value"):
        s[f"mha/{part}/kernel"] = (c, heads, d)
        s[f"mha/{part}/bias"] = (heads, d)
    return s


def layer_specs(c: int, heads: int, ff: int, blocks: int) -> dict[str, tuple]:
    return {f"block{j}/{leaf}": shp for j in range(blocks) for leaf, shp in block_specs(c, heads, ff).items()}


def _specs_of(kind: str, a: dict) -> dict[str, tuple]:
    if kind == LOCAL:
        return layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a["feed_forward_dim"]), int(a.get("num_blocks", 1)))
    return ar.layer_specs(int(a["embed_dim"]), int(a["num_heads"]), int(a.get("feed_forward_dim", 0)), bool(a.get("use_ffn", True)))


def weight_specs(cfg: dict) -> dict[str, tuple]:
    specs = dict(of.weight_specs(without_attention(cfg)))
    for i, kind, a in attention_layers(cfg):
        for leaf, shp in _specs_of(kind, a).items():
            specs[f"rep/{i}/{leaf}"] = shp
    return specs


def random_layer_weights(specs: dict[str, tuple], rng) -> dict[str, np.ndarray]:
    return ar.random_layer_weights(specs, rng)


def random_weights(cfg: dict, seed: int = 38341) -> dict[str, np.ndarray]:
    w = dict(of.random_weights(without_attention(cfg), seed))
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for i, kind, a in attention_layers(cfg):
        for leaf, v in ar.random_layer_weights(_specs_of(kind, a), rng).items():
            w[f"rep/{i}/{leaf}"] = v
    return w


# ---- the model forward --------------------------------------------------------------------------------------------------
def forward(cfg: dict, weights: dict, ids: np.ndarray, dtype=torch.float64, dead_fill: float = DEAD_FILL) -> dict[str, np.ndarray]:
    """``oracle.forward.forward`` for a model with attention layers, composed as ``attention_reference.forward`` does it.
    Behind a ``cross_frame_attention`` no mask exists; behind a ``local_attention`` the mask is KEPT - and its dead
    positions hold ``dead_fill``, not the engine's zeros: the outputs may not depend on what is there."""
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
        # (a segment's mask: _run_block returns none - re-walk the mask rule of its layers)
        mask = _mask_behind(mask, seg, cfg, dtype)
        lw = ar.sub_weights(weights, f"rep/{cut}")
        if kind == ar.ATTN:
            y = ar.cross_frame_attention(x.detach().numpy(), lw, int(a["num_heads"]), bool(a.get("use_ffn", True)))
            mask = None                                                  # the layer does not set supports_masking
        else:
            y, dead = local_attention(x.detach().numpy(), lw, int(a["num_heads"]), int(a["window_size"]), int(a.get("num_blocks", 1)),
                                      None if mask is None else mask.numpy())
            y[dead] = dead_fill
        x = torch.as_tensor(y).to(dtype)
        start = cut + 1
    out = {"embedding": x}
    logits, _ = of._run_block(x, None, cfg["classifier"]["hidden_layers"], "classifier", weights, cfg, dtype)
    out["prediction"] = logits
    if nmds:
        out["nmd"] = nmds[0] if len(nmds) == 1 else torch.cat(nmds, dim=-1)
    return {k: v.detach().numpy() for k, v in out.items()}


def _mask_behind(mask, layers, cfg, dtype):
    """The mask ``oracle.forward._run_block`` holds behind ``layers`` (it returns the tensor alone): the rules of its own
    layer functions, applied to the mask with a one-channel dummy tensor where a conv needs one."""
    use_masking_default = bool(cfg.get("use_masking", True))
    for layer in layers:
        name = layer.get("name", "").lower()
        c = dict(layer.get("config", {}) or {})
        um = c.get("use_masking", use_masking_default)
        convs = []
        if name == "masked_conv1d":
            convs = [(c["kernel_size"], c.get("strides", 1), c.get("padding", "valid"), c.get("dilation_rate", 1), c.get("mask_mode", "any"))]
        elif name == "residual_block":
            k, dil, p = c.get("kernel_size", 3), c.get("dilation_rate", 1), c.get("padding", "same")
            for j in range(c.get("block_size", 1)):
                convs += [(k, c.get("strides", 1) if j == 0 else 1, p, dil, "any"), (k, 1, p, dil, "any")]
        elif name == "masked_batchnorm" and not um:
            mask = None
        if convs and not um:
            mask = None
        for k, s, p, dil, mode in convs:
            if mask is None:
                break
            dummy = torch.zeros(mask.shape + (1,), dtype=dtype)
            _, mask = of.masked_conv1d(dummy, mask, {"kernel": torch.zeros((k, 1, 1), dtype=dtype)}, kernel_size=k, strides=s, padding=p,
                                       dilation_rate=dil, use_bias=False, use_masking=True, mask_mode=mode)
    return mask


# ---- inputs -------------------------------------------------------------------------------------------------------------
def window_ids(l: int, kind: str, n_win: int = 6, seed: int = 11, half: int = 8, grow: int = 0) -> np.ndarray:
    """(n_win, 6, l) codon ids.  ``full`` / ``ragged`` / ``few``: tests/attention_reference.py.  ``long_n``: whole windows
    with one run of invalid codons longer than ``2 half + 1`` in every row of the odd windows - dead positions in the
    interior (where l leaves no room for such a run: as long as fits, down to nothing); ``short_n``: a run shorter than
    ``2 half + 1`` - masked positions that stay live.  ``grow``: by how many positions the convs in front of the layer
    shorten an invalid run (their output masks grow): the runs are made that much longer."""
    if kind in ("full", "ragged", "few"):
        return ar.window_ids(l, kind, n_win, seed)
    assert kind in ("long_n", "short_n"), kind
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    ids = rng.integers(1, 65, (n_win, 6, l))
    run = min((2 * half + 4 if kind == "long_n" else max(half, 1)) + grow, max(l - 2, 0))
    for w in range(n_win):
        for f in range(6):
            if (w + f) % 2 == 0 and run > 0:
                a = int(rng.integers(1, l - run))
                ids[w, f, a:a + run] = 0
    return ids.astype(np.uint8)


def value_inputs(c: int, rows: int, l: int, seed: int = 5):
    """(name, x (rows, l, c) f32): unit normal; GELU-like (one-sided, a few large); rows with a common offset far above
    their spread (the layer norm's cancellation); exact zeros at half of the positions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(0, 1, (rows, l, c))
    gelu = np.maximum(x, 0) * rng.choice([1.0, 1.0, 1.0, 8.0], x.shape)
    offset = 0.05 * x + rng.normal(0, 3, (rows, l, 1))
    padded = x.copy()
    padded[:, l // 2:] = 0.0
    return [(n, v.astype(np.float32)) for n, v in (("normal", x), ("gelu-like", gelu), ("offset rows", offset), ("zero rows", padded))]


# ---- emulation of the kernel's arithmetic (csrc/jg_localattn.hip), rounding where the kernel rounds -----------------------
def fold(w: dict, heads: int) -> dict[str, np.ndarray]:
    """The host-side fold of one block, restated (``attention_reference.fold`` under this layer's names)."""
    names = {"ln1": "attn_norm", "ln2": "ffn_norm", "ffn1": "ffn_dense1", "ffn2": "ffn_dense2", "mha": "mha"}
    return ar.fold({f"{names[k.split('/', 1)[0]]}/{k.split('/', 1)[1]}": v for k, v in w.items()}, heads, True)


def blob_of(fw: dict) -> np.ndarray:
    return np.concatenate([fw[k].ravel() for k in ("wq", "wk", "wv", "bq", "bk", "bv", "wo", "bo", "w1", "b1", "w2", "b2")])


def evaluate_fold(x, fw: dict, heads: int, window: int, mask=None):
    """The folded operands evaluated plainly in float64: normalise without gamma / beta, the folded kernels and biases,
    no separate query scale - what the kernel computes, in exact arithmetic."""
    x = np.asarray(x, np.float64)
    r_, l, c = x.shape
    d = c // heads
    g = lambda k: np.asarray(fw[k], np.float64)
    m = np.broadcast_to(attention_mask(l, window, mask), (r_, l, l))
    ones, zeros = np.ones(c), np.zeros(c)
    xn = layer_norm(x, ones, zeros)
    q, k, v = ((xn @ g("w" + p) + g("b" + p)).reshape(r_, l, heads, d) for p in "qkv")
    s = np.where(m[:, None], np.einsum("rqhd,rkhd->rhqk", q, k), -np.inf)
    mx = s.max(axis=-1, keepdims=True)
    e = np.where(m[:, None], np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
    tot = e.sum(axis=-1, keepdims=True)
    ctx = np.einsum("rhqk,rkhd->rqhd", e / np.where(tot > 0, tot, 1.0), v).reshape(r_, l, c)
    t = x + ctx @ g("wo") + g("bo")
    t = t + gelu_tanh(layer_norm(t, ones, zeros) @ g("w1") + g("b1")) @ g("w2") + g("b2")
    t[~m.any(axis=-1)] = 0.0
    return t


def emulate_block(x, w: dict, heads: int, window: int, mask=None) -> np.ndarray:
    """The kernel's arithmetic in numpy: f32 everywhere, one rounding where the kernel has one.  x (R, L, C)."""
    x = np.asarray(x, f32)
    r_, l, c = x.shape
    d = c // heads
    half = window // 2
    fw = fold(w, heads)
    ok = np.ones((r_, l), bool) if mask is None else np.asarray(mask, bool)
    t = x.reshape(-1, c)
    n_tok = t.shape[0]
    xn = ar._ln32(t, LN_EPS)
    q, k, v = (ar._fma_chain(np.broadcast_to(fw["b" + p], (n_tok, c)).astype(f32), xn, fw["w" + p]).reshape(r_, l, heads, d) for p in "qkv")
    sp = 2 * half + 1
    padk = lambda a: np.concatenate([np.zeros((r_, half) + a.shape[2:], a.dtype), a, np.zeros((r_, half) + a.shape[2:], a.dtype)], axis=1)
    kp, vp, okp = padk(k), padk(v), padk(ok)
    s = np.zeros((r_, l, heads, sp), f32)
    val = np.zeros((r_, l, sp), bool)
    for dj in range(sp):                                                  # key q - half + dj
        kk = kp[:, dj:dj + l]
        acc = np.zeros((r_, l, heads), np.float64)
        for i in range(d):
            acc = (acc + q[..., i].astype(np.float64) * kk[..., i].astype(np.float64)).astype(f32).astype(np.float64)
        s[..., dj] = acc.astype(f32)
        val[..., dj] = okp[:, dj:dj + l]
    vm = val[:, :, None, :]
    mx = np.where(vm, s, -np.inf).max(axis=-1, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, f32(0.0)).astype(f32)
    e = np.where(vm, np.exp2(((s - mx).astype(f32) * f32(1.44269504)).astype(f32)), f32(0.0)).astype(f32)
    tot = np.zeros(e.shape[:-1], f32)
    for dj in range(sp):
        tot = (tot + e[..., dj]).astype(f32)
    with np.errstate(divide="ignore"):
        inv = np.where(tot > 0, f32(1.0) / tot, f32(0.0)).astype(f32)
    ctx = np.zeros((r_, l, heads, d), f32)
    for i in range(d):
        acc = np.zeros((r_, l, heads), np.float64)
        for dj in range(sp):
            vv = vp[:, dj:dj + l, :, i].astype(np.float64)
            acc = (acc + e[..., dj].astype(np.float64) * vv).astype(f32).astype(np.float64)
        ctx[..., i] = (acc.astype(f32) * inv).astype(f32)
    t = ar._fma_chain((t + fw["bo"]).astype(f32), ctx.reshape(n_tok, c), fw["wo"])
    xn = ar._ln32(t, LN_EPS)
    h = ar._gelu32(ar._fma_chain(np.broadcast_to(fw["b1"], (n_tok, fw["b1"].shape[0])).astype(f32), xn, fw["w1"]))
    t = ar._fma_chain((t + fw["b2"]).astype(f32), h, fw["w2"]).reshape(r_, l, c)
    t[~val.any(axis=-1)] = 0.0
    return t


def emulate(x, w: dict, heads: int, window: int, blocks: int, mask=None) -> np.ndarray:
    """``blocks`` emulated blocks on x (B, 6, L, C), mask (B, 6, L) or None."""
    x = np.asarray(x, f32)
    b_, fr, l, c = x.shape
    t = x.reshape(b_ * fr, l, c)
    mk = None if mask is None else np.asarray(mask).reshape(b_ * fr, l) != 0
    for j in range(blocks):
        t = emulate_block(t, ar.sub_weights(w, f"block{j}"), heads, window, mk)
    return t.reshape(b_, fr, l, c)


# ---- the per-op bound, over the live positions -----------------------------------------------------------------------------
def live_errors(got, ref, dead) -> tuple[float, float]:
    live = ~np.asarray(dead, bool)
    return ar.errors(np.asarray(got)[live], np.asarray(ref)[live])


def bounds_from(emu, ref, dead) -> dict:
    live = ~np.asarray(dead, bool)
    return ar.bounds_from(np.asarray(emu)[live], np.asarray(ref)[live])


# ---- the fixture model ----------------------------------------------------------------------------------------------------
FIXTURE = dict(embed_dim=32, num_heads=4, feed_forward_dim=128, window_size=16, num_blocks=2, dropout_rate=0.1)


def fixture_cfg(crossframe_cfg: dict, **over) -> dict:
    """tests/golden/crossframe500_project.yaml's model with its attention layer swapped for ``local_attention`` (FIXTURE,
    updated by ``over``)."""
    cfg = copy.deepcopy(crossframe_cfg)
    layers = cfg["representation_learner"]["hidden_layers"]
    at = [i for i, layer in enumerate(layers) if layer["name"] == ar.ATTN][0]
    layers[at] = {"name": LOCAL, "config": {**FIXTURE, **over}}
    return cfg
