"""Shared cases of the per-op parity checks (tests/test_op_reference.py on the CPU, tests/test_gpu_op_taps.py on the GPU):
the model variants, id tensors whose masks change at tile edges and row ends, the element-wise error check against the
float64 op reference (oracle/ops.py), and a numpy emulation of the split-f16 conv arithmetic with the mutations the
check must catch.

The check.  For a conv (or element-wise op) with float64 reference ``ref`` and magnitude ``M`` (oracle/ops.py: the linear
part on |x|, |W|, through |BN scale|, plus |residual|, times each activation's Lipschitz constant) every element obeys

    |got - ref| <= GAMMA * M + 2^-21 |ref| + 2^-24

(the 2^-24 floor: an F16S value below 2^-3 has a subnormal lo part), and the op's RMS of |got - ref| / M_rms stays at or
below RMS_BOUND - a precision-class bug (a product term dropped everywhere) can hide under the element bound, not under this.
Only for an F16S-stored element with |ref| < 2^-3 - its lo part is subnormal, so storing it rounds by up to 2^-25 absolute
- that storage rounding is taken off the error first: the RMS runs over max(|got - ref| - 2^-25, 0) / M there, over
|got - ref| / M everywhere else; any error beyond the format's own rounding counts in full.  The legacy tower's real weights
have a channel whose BN scale is 1.1e-5 (outputs near 2.6e-4, M near 2.7e-4), where the storage quantum alone is err / M ~
1e-4 - on the GPU that channel stays inside the element bound (worst err / bound 0.48) but fails an RMS taken over err / M.

Constants, from the emulation below on brain's first block conv2 (k = 5, dilation 3, 128 -> 128, BN + residual + GELU;
tests/test_op_reference.py::test_checker_bounds_sit_between_emulation_and_mutations re-measures the margins every run):

    GAMMA     = 6e-6      largest emulated err / M 1.9e-7                       -> 32x above it (>= 4x required)
                          smallest mutation (hi_x lo_w dropped) err / M 5.7e-5   -> 9.5x below it (>= 8x required); the
                          other mutations reach err / M 0.07 - 0.48
    RMS_BOUND = 2^-21     emulated RMS 1.1e-8 -> 42x above it; the dropped cross term's RMS 7.4e-6 -> 15x below it.
                          The same conv scaled down 2^-8 (test_checker_on_a_small_magnitude_op): emulated RMS 1.3e-7 (3.6x:
                          the input's own lo parts turn subnormal there), the dropped cross term 4.9e-6 (10x)
"""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

GAMMA = 6e-6
RMS_BOUND = 2.0 ** -21
REL = 2.0 ** -21
FLOOR = 2.0 ** -24


# ---- models -------------------------------------------------------------------------------------------------------
def model_cfg(name: str) -> dict:
    """A ``*_project.yaml`` model or one of the variants: ``pyramid_k7`` / ``pyramid_k9`` (7- / 9-tap blocks), ``brain_ln``
    (MaskedLayerNormalization blocks), ``zeus_mixed`` (the last residual stack unmasked), ``brain_majority`` / ``brain_strict`` (mask modes), ``baseline500_dicodon_pos``
    (dicodon ids and positional embeddings)."""
    from conftest import load_model_cfg
    base = name.split("_")[0]
    cfg = copy.deepcopy(load_model_cfg(base))
    variant = name[len(base) + 1:]
    layers = cfg["representation_learner"]["hidden_layers"]
    if variant in ("k7", "k9"):
        k = int(variant[1])
        for layer in layers:
            if layer["name"] == "residual_block":
                layer["config"]["kernel_size"] = k
                layer["config"]["dilation_rate"] = min(int(layer["config"].get("dilation_rate", 1)), 64 // (k - 1))
    elif variant == "ln":
        for layer in layers:
            if layer["name"] == "residual_block":
                layer["config"]["norm_type"] = "masked_layernorm"
    elif variant == "mixed":
        # the last residual stack without masking: its DyT epilogues run without the mask, the others with it
        [blk for blk in layers if blk["name"] == "residual_block"][-1]["config"]["use_masking"] = False
    elif variant in ("majority", "strict"):
        for layer in layers:
            if layer["name"] in ("masked_conv1d", "residual_block"):
                layer["config"]["mask_mode"] = variant
    elif variant == "dicodon_pos":
        cfg["string_processor"]["codon"], cfg["string_processor"]["codon_id"] = "DICODON", "DICODON_ID"
        cfg["embedding"]["embedding_size"] = 16
        cfg["embedding"]["use_positional_embeddings"] = True
        cfg["embedding"]["positional_embedding_length"] = 10000
    elif variant:
        raise ValueError(name)
    return cfg


#: kernel gain of the stand-in weights (deep stacks of He-uniform kernels otherwise drive activations far out)
GAIN = {"pyramid": 0.85, "pyramid_k7": 0.7, "pyramid_k9": 0.7}


def weights_for(name: str, cfg: dict, seed: int = 38341) -> dict:
    from oracle import forward as ofwd
    w = ofwd.random_weights(cfg, seed=seed)
    g = GAIN.get(name)
    if g is not None:
        for key in w:
            if key.startswith("rep/") and key.endswith("/kernel"):
                w[key] = w[key] * np.float32(g)
    return w


def compile_model(name: str, seed: int = 38341):
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    cfg = model_cfg(name)
    w = weights_for(name, cfg, seed)
    return cfg, w, compile_plan(build_plan(cfg), w)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def edge_ids(l: int, n_win: int = 12, vocab: int = 65, seed: int = 5, fsize_codons: int | None = None) -> np.ndarray:
    """(n_win, 6, l) ids: random valid codons with N runs (id 0) placed where masks change at the 256-position tile edge
    (codons 250 - 262), at row starts and at row ends; ragged windows shorter than the row; one all-N window.  Base index =
    3 codon + frame for the forward frames; the reverse frames mirror it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(1, vocab, (n_win, 6, l))
    n_bases = 3 * l + 2
    for w in range(n_win):
        bases_n = np.zeros(n_bases, bool)
        if w % 4 == 0:
            a = 250 + (w // 4) % 12                      # one run per window, ending at a different codon of 250 .. 262
            bases_n[3 * a: 3 * a + 2 + w % 3] = True
        if w % 4 == 1:
            bases_n[: 1 + 3 * (w % 5)] = True            # row start
            bases_n[n_bases - 1 - 3 * (w % 7):] = True   # row end
        if w % 4 == 2:
            bases_n[3 * 255: 3 * 257] = True             # straddles the edge
        for f in range(3):
            codon_n = np.array([bases_n[3 * c + f: 3 * c + f + 3].any() for c in range(l)])
            ids[w, f, codon_n] = 0
            ids[w, 3 + f, codon_n[::-1]] = 0
    for w in (3, 7):                                     # ragged: the window ends early (padding = id 0)
        if w < n_win:
            cut = l - 37 * (w + 1) if l > 300 else l // 2
            ids[w, :, cut:] = 0
    if n_win > 10:
        ids[10] = 0                                      # all N
    return ids.astype(np.uint16 if vocab > 256 else np.uint8)


# ---- the check ----------------------------------------------------------------------------------------------------
@dataclass
class CheckResult:
    worst: float          # max err / bound over elements (<= 1 passes)
    worst_m: float        # max err / M
    rms: float            # RMS of err / M (less the F16S storage rounding where the lo part is subnormal)
    n_bad: int
    offenders: list       # (window, frame, position, position mod 256, channel, err / M)

    @property
    def ok(self) -> bool:
        return self.n_bad == 0 and self.rms <= RMS_BOUND

    def report(self, what: str) -> str:
        return (f"{what}: worst err/bound {self.worst:.3g}, worst err/M {self.worst_m:.3g} (GAMMA {GAMMA:.3g}), "
                f"rms err/M {self.rms:.3g} (bound {RMS_BOUND:.3g}), {self.n_bad} elements out"
                + ("" if self.ok else "; worst (window, frame, pos, pos % 256, channel, err/M): " + str(self.offenders)))


def check(got: np.ndarray, ref: np.ndarray, M: np.ndarray, gamma: float = GAMMA, windows_per_row: int = 1,
          f16s: bool = False) -> CheckResult:
    """``f16s``: ``got`` was stored as F16S (hi + lo f16 pairs): elements below 2^-3 sit on the 2^-24 storage quantum."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bound = gamma * M + REL * np.abs(ref) + FLOOR
    ratio = err / bound
    rel = err / np.maximum(M, FLOOR)
    sub = (np.abs(ref) < 2.0 ** -3) if f16s else np.zeros(ref.shape, bool)
    rel_floor = np.maximum(err - np.where(sub, 2.0 ** -25, 0.0), 0.0) / np.maximum(M, FLOOR)
    bad = ratio > 1.0
    flat = np.argsort(rel, axis=None)[::-1][:6]
    offenders = []
    for f in flat:
        idx = np.unravel_index(f, rel.shape)
        r, fr, p = int(idx[0]), int(idx[1]), int(idx[2])
        ch = int(idx[3]) if len(idx) > 3 else 0
        offenders.append((r // windows_per_row, fr, p, p % 256, ch, float(rel[idx])))
    return CheckResult(float(ratio.max()), float(rel.max()), float(np.sqrt((rel_floor ** 2).mean())), int(bad.sum()), offenders)


# ---- split-f16 emulation and mutations ----------------------------------------------------------------------------
def split16(a: np.ndarray, scale: float = 1.0):
    """f32 -> (hi, lo) numpy f16 pair (scaled by a power of two, as the kernels pre-scale the weights)."""
    a = np.asarray(a, np.float32) * np.float32(scale)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def resplit(y: np.ndarray) -> np.ndarray:
    """An f32 result stored as F16S and read back: hi + lo in f32."""
    hi, lo = split16(y)
    return hi.astype(np.float32) + lo.astype(np.float32)


def emulate_conv(program, i: int, state, drop_cross: bool = False) -> np.ndarray:
    """Op ``i`` (a conv) in the split-f16 arithmetic: operands as f16 hi / lo pairs, the products hi_x hi_w + lo_x hi_w +
    hi_x lo_w (each exact in f32) accumulated in f32 tap by tap, the epilogue in f32, the result re-split to F16S.
    ``drop_cross``: leave out hi_x lo_w (a mutation)."""
    from oracle import ops
    op = program.ops[i]
    x = ops.conv_input(program, op, state).astype(np.float32)
    w = ops.conv_weights(program, op).astype(np.float32)
    sw = 2.0 ** 10                                              # keeps the weights' lo parts out of the f16 subnormals
    xh, xl = split16(x)
    wh, wl = split16(w, sw)
    lo_, pl = ops.conv_geometry(x.shape[-2], op.k, op.stride, op.dilation, op.padding)
    y = np.zeros(x.shape[:-2] + (lo_, op.cout), np.float32)
    m = np.arange(lo_)
    f = np.float32
    for t in range(op.k):
        src = m * op.stride + t * op.dilation - pl
        ok = (src >= 0) & (src < x.shape[-2])
        a_h, a_l = xh[..., src[ok], :].astype(f), xl[..., src[ok], :].astype(f)
        acc = a_h @ wh[t].astype(f) + a_l @ wh[t].astype(f)
        if not drop_cross:
            acc = acc + a_h @ wl[t].astype(f)
        y[..., ok, :] += acc.astype(f)
    y = (y / f(sw)).astype(f)
    v, _, _ = ops._stages(program, op, y.astype(np.float64), np.zeros_like(y, np.float64), state)
    return resplit(v.astype(np.float32)).astype(np.float64)


def tap_contribution(program, i: int, state, t: int, rows=slice(None), positions=None, shift: int = 0) -> np.ndarray:
    """Tap t's term of conv op i at the given output positions, the input read ``shift`` positions off."""
    from oracle import ops
    op = program.ops[i]
    x = ops.conv_input(program, op, state)
    w = ops.conv_weights(program, op)
    lo_, pl = ops.conv_geometry(x.shape[-2], op.k, op.stride, op.dilation, op.padding)
    y = np.zeros(x.shape[:-2] + (lo_, op.cout))
    for p in positions:
        src = p * op.stride + t * op.dilation - pl + shift
        if 0 <= src < x.shape[-2]:
            y[rows, :, p, :] = x[rows, :, src, :] @ w[t]
    return y
