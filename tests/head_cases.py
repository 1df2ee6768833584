"""Shared cases of the vector head's checks (tests/test_head_reference.py on the CPU, tests/test_gpu_head.py on the GPU): every
kernel behind the pool - ``pool_kernel``, ``nmd_final_kernel``, the three dense kernels (``dense_kernel``,
``dense_narrow_kernel<8>``, ``dense_tiled_kernel<8>``), ``vecmax_kernel``, ``oodsig_kernel``, ``strand_merge_kernel`` - against
oracle/ops.py's float64 evaluation of that ONE op from the values the GPU itself fed it.

The method: sibling models.  A head's inner vectors live in hidden slots without a readback, but forwards are bit-repeatable, so
the hidden slot of one model is the exposed output of a sibling compiled from the SAME weight dict:

* a head prefix - the head cut after layer j exposes layer j's output as ``prediction``;
* ``merge: concat`` - the raw tap vectors as ``nmd`` (same representation learner as the ``max`` model);
* strand-merge ``concat`` - the per-strand head vectors as ``prediction``;
* an identity head - kernel ``eye``, no bias: products with 0 and 1 are exact, so it exposes ``embedding`` (per strand) or
  ``[nmd | signals]`` bit for bit (tests/kat_models.py::ood_signal_case's technique).

Layers that would otherwise want the same weight name in two siblings (a reliability head behind 48 raw or 10 merged channels)
sit at different positions of their YAML lists (``_at``: dropout layers in front), so ONE dict serves the family.  The premise is
asserted wherever it shows (``embedding`` / ``nmd`` bit-identical between siblings, equal op fields and weight bytes of the
shared layer, the same kernel by the restated launch rule); a broken premise can only make a check fail.

The check is op_cases.check / fused_cases.check_vec:  |got - ref| <= gamma M + 2^-21 |ref| + 2^-24  and  RMS(err / M) <= rms.

Bounds.  An f32 sum of n addends is bounded by the format whatever the order: gamma = n 2^-24, RMS <= (sqrt(n) + 1) 2^-24
(``gamma_sum`` / ``rms_sum``: a dense layer of cin inputs has n = cin + 1, a pool / tap mean n = positions); M carries the
activation's Lipschitz constant (oracle/ops.py).  A maximum of given values, the strand merge of two rows, an identity head and a
forward under another chunk are exact: bit equality.  What the format does not give - ``v_exp_f32`` / ``v_rcp_f32`` in GELU and
sigmoid, ``tanhf``, ``expf`` / ``logf`` / ``sqrtf`` in the signals - is measured on numpy float32 emulations of the kernels as
their source states them (the three dense summation orders, the signal formulas in the kernel's order), on this module's own
cases, and set >= 4x above the largest emulated error, rounded up to a power of two; every mutation below must then sit >= 8x
beyond the bounds.  tests/test_head_reference.py::test_bounds_sit_between_emulation_and_mutations re-measures both on every run.

Measured (the CPU tier prints them; 13 windows of 40 codons - the NMD / pool cases also 3 codons -, the cases of this module,
each dense layer in one launch group and in groups of 5, 5, 3):

    dense, linear / relu        : the format bound alone.  Emulation: err / bound <= 0.054 (18x inside), RMS <= its bound / 13
    ACT_GAMMA[gelu]    = 2^-21    the activation alone (act32 against float64 on the same f32 sums): largest err / M 6.3e-8
                                  -> 7.5x; the whole layer 33x (element) and 40x (RMS) inside
    ACT_GAMMA[tanh]    = 2^-21    activation alone 8.2e-8 -> 5.8x; whole layer 28x / 51x
    ACT_GAMMA[sigmoid] = 2^-20    activation alone 1.3e-7 (half an ulp of an output near 1 / 2 over M = 1 / 2) -> 7.4x; whole
                                  layer 42x / 55x
    ACT_RMS            = ACT_GAMMA / 4 (the RMS headrooms above are with it)
    vecmax                      : the block-diagonal dense layer's bound; 23x / 22x inside and more
    SIG_GAMMA = 2^-21           the five signals: largest emulated err / M 1.03e-7 (entropy over seven classes) -> 4.6x, the
                                  smallest power of two that leaves 4x; the emulation sits 7.8x inside the element bound
    SIG_RMS   = 2^-22           emulated RMS 2.98e-8 -> 8x.  2^-23 would leave 4.0004x: less than libm's exp / log differ
                                  between builds, so the CPU tier's own 4x assertion would hang on the numpy at hand
    NMD finish                  : format bound alone; 8.1x / 8.8x inside (tap sums one partial row per frame, then the finish)
    pool, average               : format bound alone; 6.7x / 4.2x inside (500 channels: two position groups of 120 terms)
    pool, max; strand merge; identity heads; another chunk: bit equality (the max pool on the device: asserted in
    tests/test_gpu_head.py beside part D's loop, whose check alone would leave 2^-21 |ref| + 2^-24)
    mutations: the nearest is "weights read at the padded pitch" on a 500 -> 77 tanh layer, 1.9e4x beyond its bound; the others
    3e4x and more, or not finite (energy without the max shift overflows at +88.5; the NMD finish without eps is 0 / 0 at the
    all-N window).  "Padded cin lanes hold the next window's first inputs" shows only because the mutation ALSO drops the
    kernel's weight guard (``i + c < cin ? w : 0``) and reads what follows the matrix in the blob: with the guard kept, as in
    dense_tiled_kernel, the lanes multiply zeros and no check can see what they hold.

On an MI355X (tests/test_gpu_head.py, 52 tests, 1 s): dense err / bound <= 0.062, vecmax <= 0.03, signals <= 0.16, pool average <=
0.11, NMD finish <= 0.13; every bit equality holds.  No kernel bug found.
"""
from __future__ import annotations

import copy
import math

import numpy as np

import fused_cases as fc
import op_cases as oc

F = np.float32
WT = 8                      # windows per workgroup of dense_tiled_kernel<8>
ROWS, CHUNK, CODONS = 13, 5, 40

ACT_GAMMA = {"gelu": 2.0 ** -21, "tanh": 2.0 ** -21, "sigmoid": 2.0 ** -20}
ACT_RMS = {k: v / 4 for k, v in ACT_GAMMA.items()}
SIG_GAMMA = 2.0 ** -21
SIG_RMS = 2.0 ** -22


# ---- format-derived bounds (tests/test_gpu_fused_kernels.py part D) ---------------------------------------------------------
#: An f32 sum of n addends: |error| <= (n - 1) 2^-24 x (sum of |addends|) whatever the order, and the pooled mean's M is that sum
#: over the count: gamma = n 2^-24 bounds a pool / tap mean of n positions (a dense layer of n inputs: n + 1 addends); rounding
#: errors of independent additions add up like a random walk: RMS <= (sqrt(n) + 1) 2^-24.  Split-f16: a sum taken in the conv
#: kernel sees the values before they are stored as F16S (hi + lo keeps 22 bits): + 2^-21 on both.  A maximum of stored values is
#: exact.
def gamma_sum(n: int, precision: str = "f32") -> float:
    return n * 2.0 ** -24 + (2.0 ** -21 if precision == "f16x3" else 0.0)


def rms_sum(n: int, precision: str = "f32") -> float:
    return (n ** 0.5 + 1.0) * 2.0 ** -24 + (2.0 ** -21 if precision == "f16x3" else 0.0)


def _act_name(code: int):
    from oracle import ops
    return {ops.ACT_NONE: None, ops.ACT_RELU: "relu", ops.ACT_GELU_TANH: "gelu", ops.ACT_TANH: "tanh", ops.ACT_SIGMOID: "sigmoid"}[code]


def dense_bounds(cin: int, act_code: int) -> tuple:
    """(gamma, rms bound) of a dense layer of ``cin`` inputs behind activation ``act_code`` (M carries the Lipschitz constant)."""
    name = _act_name(act_code)
    return gamma_sum(cin + 1) + ACT_GAMMA.get(name, 0.0), rms_sum(cin + 1) + ACT_RMS.get(name, 0.0)


# ---- the launch rule of jg_launch_dense, restated -----------------------------------------------------------------------------
def dense_kernel(rows: int, cin: int, cout: int) -> str:
    """Which kernel a dense layer of (cin -> cout) runs on in a launch group of ``rows`` rows (jg_kernels.hip jg_launch_dense)."""
    if cout >= 64 and cin >= 64 and rows >= WT and WT * ((cin + 3) & ~3) * 4 <= 48 * 1024:
        return "tiled"
    if cout <= 8 and cin >= 64:
        return "narrow"
    return "plain"


def groups_of(n: int, chunk: int) -> list:
    chunk = chunk or n
    return [min(chunk, n - r0) for r0 in range(0, n, chunk)]


# ---- configs --------------------------------------------------------------------------------------------------------------
_SP = {"data_format": "numpy", "seq_onehot": False, "codon": "CODON", "codon_id": "CODON_ID", "crop_size": 100}
_DROP = {"name": "dropout", "config": {"rate": 0.1}}


def _conv(width: int, bias: bool = True) -> dict:
    return {"name": "masked_conv1d", "config": {"filters": width, "kernel_size": 3, "padding": "same", "use_bias": bias}}


def _dense(units: int, act=None, bias: bool = True) -> dict:
    return {"name": "dense", "config": {"units": units, "activation": act, "use_bias": bias}}


def _at(index: int, layer: dict) -> list:
    """``layer`` at position ``index`` of a YAML list (dropout layers in front): its weights are named ``<head>/<index>/...``."""
    return [copy.deepcopy(_DROP) for _ in range(index)] + [layer]


def translated_cfg(rep: list, head: list, pooling: str = "max", e: int = 4, masked: bool = True, rel: dict | None = None) -> dict:
    n_out = [ly for ly in head if ly["name"] == "dense"][-1]["config"]["units"]
    width = [ly for ly in rep if ly["name"] == "masked_conv1d"][-1]["config"]["filters"]
    cfg = {"name": "head", "classifier_out_dim": n_out, "use_masking": masked,
           "class_label_map": [{"class": f"c{i}", "label": i} for i in range(n_out)],
           "embedding": {"use_embedding_layer": True, "input_type": "translated", "strands": 2, "frames": 6,
                         "input_shape": [6, None], "embedding_size": e},
           "string_processor": dict(_SP),
           "representation_learner": {"hidden_layers": copy.deepcopy(rep), "pooling": pooling},
           "classifier": {"input_shape": width, "hidden_layers": copy.deepcopy(head)}}
    if rel is not None:
        cfg["reliability_model"] = copy.deepcopy(rel)
    return cfg


def shared_weights(cfgs: list, seed: int = 38341, strands: bool = False) -> dict:
    """ONE weight dict for a family: the first config's seeded weights, then whatever names the others add.  A name two siblings
    share must have one shape."""
    from oracle import forward as ofwd
    from oracle import strands as ost
    w = {}
    for q, cfg in enumerate(cfgs):
        for k, v in (ost if strands else ofwd).random_weights(cfg, seed=seed + q).items():
            if k in w:
                assert w[k].shape == v.shape, (k, w[k].shape, v.shape)
            else:
                w[k] = v
    return w


def compile_cfg(cfg: dict, w: dict):
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    return compile_plan(build_plan(cfg), w)


class Family:
    """Sibling models from one weight dict: ``cfgs`` name -> config, ``w`` the dict, ``progs`` name -> program."""

    def __init__(self, cfgs: dict, overrides: dict | None = None, strands: bool = False, seed: int = 38341):
        self.cfgs = cfgs
        self.strands = strands
        self.w = shared_weights(list(cfgs.values()), seed, strands)
        for k, v in (overrides or {}).items():
            assert k in self.w and self.w[k].shape == v.shape, (k, v.shape)
            self.w[k] = np.asarray(v, np.float32)
        self.progs = {k: compile_cfg(c, self.w) for k, c in cfgs.items()}


def head_chain(prog, out_vec: int) -> list:
    """Indices of the dense ops that end in vector slot ``out_vec``, first layer first."""
    from oracle import ops
    chain = []
    want = out_vec
    for i in range(len(prog.ops) - 1, -1, -1):
        op = prog.ops[i]
        if op.kind == ops.OP_DENSE and op.out_vec == want and (chain or want == out_vec):
            chain.append(i)
            want = op.in_vec
            if want in (ops.VEC_EMBEDDING, ops.VEC_NMD):
                break
    return chain[::-1]


def op_fields(prog, i: int) -> tuple:
    """What makes two dense ops the same layer: shape, activation, bias or none, and the weight bytes."""
    op = prog.ops[i]
    blob = np.asarray(prog.blob, np.float32)
    return (op.kind, op.cin, op.cout, op.arg, op.b_off >= 0, blob[op.w_off:op.w_off + op.cin * op.cout].tobytes(),
            blob[op.b_off:op.b_off + op.cout].tobytes() if op.b_off >= 0 else b"")


# ---- 1. dense ---------------------------------------------------------------------------------------------------------------
#: family -> (conv width, [(units, activation)]): every (cin -> cout) of DENSE_WANT is some layer of some family
DENSE_FAMILIES = {
    "w68_a": (68, [(500, "gelu"), (77, "tanh"), (257, "sigmoid"), (3, None)]),
    "w68_b": (68, [(500, "relu"), (6, "sigmoid")]),
    "w68_c": (68, [(77, "gelu"), (9, None)]),
    "w68_d": (68, [(100, "relu"), (1, "tanh")]),
    "w64_a": (64, [(64, "relu"), (1536, "tanh"), (64, None), (8, "gelu")]),
    "w64_b": (64, [(1540, "sigmoid"), (64, "gelu"), (8, None)]),
    "w60": (60, [(8, "relu")]),
    "w64": (64, [(8, "tanh")]),
    "w68": (68, [(500, None)]),
}
#: (cin, cout) -> the kernel the shape is there for in ONE launch group of 13 windows
DENSE_WANT = {(68, 500): "tiled", (500, 77): "tiled", (77, 257): "tiled", (64, 64): "tiled", (1536, 64): "tiled",
              (1540, 64): "plain", (77, 9): "plain", (60, 8): "plain",
              (257, 3): "narrow", (64, 8): "narrow", (100, 1): "narrow", (500, 6): "narrow"}
DENSE_ACTS = {None, "gelu", "relu", "tanh", "sigmoid"}


def dense_family(name: str, bias: bool = True) -> Family:
    """The head of DENSE_FAMILIES[name] and its prefixes (key = number of layers kept) behind one 3-tap conv and the max pool."""
    width, layers = DENSE_FAMILIES[name]
    head = [_dense(u, a, bias) for u, a in layers]
    cfgs = {j: translated_cfg([_conv(width)], head[:j]) for j in range(len(head), 0, -1)}
    return Family(cfgs)


def dense_reference(prog, i: int, x: np.ndarray):
    """Dense op ``i`` in float64 from input rows ``x`` -> (ref, M, gamma, rms bound)."""
    from oracle import ops
    op = prog.ops[i]
    st = ops.State(np.zeros((len(x), 1, 1), np.uint8))
    st.vec[op.in_vec] = np.asarray(x, np.float64)
    ref = ops.run_op(prog, i, st).out
    blob = np.asarray(prog.blob, np.float64)
    mag = np.abs(np.asarray(x, np.float64)[:, :op.cin]) @ np.abs(blob[op.w_off:op.w_off + op.cin * op.cout]).reshape(op.cin, op.cout)
    if op.b_off >= 0:
        mag = mag + np.abs(blob[op.b_off:op.b_off + op.cout])
    mag = mag * ops.LIPSCHITZ[op.arg] + (0.5 if op.arg == ops.ACT_SIGMOID else 0.0)
    return (ref, mag) + dense_bounds(op.cin, op.arg)


def check_dense(prog, i: int, x: np.ndarray, got: np.ndarray):
    ref, mag, gamma, rms = dense_reference(prog, i, x)
    res, ok = fc.check_vec(np.asarray(got)[:, :prog.ops[i].cout], ref, mag, gamma, rms)
    return res, ok, gamma, rms


def _fma(acc, x, w):
    """fmaf: the product of two f32 is exact in f64; one rounding of the sum to f64 first moves the f32 result by < 2^-29 ulp."""
    return (acc.astype(np.float64) + x.astype(np.float64) * w.astype(np.float64)).astype(F)


def act32(code: int, v: np.ndarray) -> np.ndarray:
    """jg_apply_act (jg_mixer_dev.h) in f32, step by step."""
    from oracle import ops
    v = np.asarray(v, F)
    with np.errstate(over="ignore"):
        if code == ops.ACT_GELU_TANH:
            a = ((F(0.10294324) * v).astype(F) * v).astype(F)
            t = (v * (F(-2.3022082) - a).astype(F)).astype(F)
            return (v * (F(1.0) / (F(1.0) + np.exp2(t).astype(F)).astype(F)).astype(F)).astype(F)
        if code == ops.ACT_RELU:
            return np.maximum(v, F(0.0))
        if code == ops.ACT_TANH:
            return np.tanh(v).astype(F)
        if code == ops.ACT_SIGMOID:
            t = (F(-1.4426950) * v).astype(F)
            return (F(1.0) / (F(1.0) + np.exp2(t).astype(F)).astype(F)).astype(F)
    assert code == ops.ACT_NONE, code
    return v


def emulate_dense(prog, i: int, x: np.ndarray, chunk: int = 0, mut: str | None = None, preact: bool = False) -> np.ndarray:
    """Dense op ``i`` as the kernel the launch rule picks for each launch group of ``chunk`` rows computes it, in numpy f32:

    plain   one thread per output: fmaf over the inputs in turn, + bias, activation;
    tiled   the same sums in the same order, the inputs from an LDS tile of 8 windows x cin padded to 4 (zeros);
    narrow  one wave per window: lane l takes inputs l, l + 64, ...; a butterfly (xor 32 ... 1) adds the 64 partial sums.

    ``mut``: one of DENSE_MUTATIONS.  ``preact``: the f32 sums in front of the activation."""
    op = prog.ops[i]
    cin, cout = op.cin, op.cout
    blob = np.asarray(prog.blob, F)

    def wat(idx):                                  # the blob at flat indices (zeros beyond its end)
        idx = np.asarray(idx)
        return np.where(idx < blob.size, blob[np.minimum(idx, blob.size - 1)], F(0))
    pitch_w = (cout + 3) & ~3 if mut == "weights read at the padded pitch" else cout
    w = wat(op.w_off + np.arange(cin)[:, None] * pitch_w + np.arange(cout)[None, :])
    b = blob[op.b_off:op.b_off + cout] if op.b_off >= 0 else None
    if b is not None and mut == "bias taken from lane o mod 8":
        b = b[np.arange(cout) % 8]
    pitch_x = (cin + 3) & ~3
    xs = np.zeros((len(x), pitch_x), F)
    xs[:, :cin] = np.asarray(x, F)[:, :cin]
    out = np.zeros((len(x), cout), F)
    r0 = 0
    for nw in groups_of(len(x), chunk):
        xg = xs[r0:r0 + nw]
        if mut == "input read at cin instead of the slot pitch":
            xg = xg.ravel()[np.arange(nw)[:, None] * cin + np.arange(pitch_x)[None, :]]
        kern = dense_kernel(nw, cin, cout)
        if kern == "narrow":
            acc = np.zeros((nw, 64, cout), F)
            for s0 in range(0, cin, 64):
                n = min(64, cin - s0)
                acc[:, :n] = _fma(acc[:, :n], xg[:, s0:s0 + n, None], w[None, s0:s0 + n])
            lane = np.arange(64)
            for d in (32, 16, 8, 4, 2, 1):
                acc = (acc + acc[:, lane ^ d]).astype(F)
            acc = acc[:, 0]
        else:
            acc = np.zeros((nw, cout), F)
            for q in range(cin):
                acc = _fma(acc, xg[:, q, None], w[None, q])
            if kern == "tiled" and mut == "padded cin lanes hold the next window's first inputs":
                # (and the weight guard gone with the zero fill: the kernel rows behind the matrix are what follows in the blob)
                nxt = np.zeros_like(xg)
                nxt[:-1] = xg[1:]
                nxt[WT - 1::WT] = 0                # (the tile's last window has no next one)
                for q in range(cin, pitch_x):
                    acc = _fma(acc, nxt[:, q - cin, None], wat(op.w_off + q * cout + np.arange(cout))[None])
        v = acc if b is None else (acc + b).astype(F)
        res = v if preact else act32(op.arg, v)
        if kern == "tiled" and mut == "tiled tail windows left unwritten":
            res[nw // WT * WT:] = 0
        out[r0:r0 + nw] = res
        r0 += nw
    return out


DENSE_MUTATIONS = ("tiled tail windows left unwritten", "padded cin lanes hold the next window's first inputs",
                   "bias taken from lane o mod 8", "weights read at the padded pitch", "input read at cin instead of the slot pitch")


# ---- 2. POOL and NMD finish, unfused ------------------------------------------------------------------------------------------
POOL_WIDTHS = (24, 40, 68, 96, 500)


def pool_cfg(width: int, pooling: str, masked: bool) -> dict:
    """One 3-tap conv with an NMD tap as its last stage, the pool, single dense heads: every op of the vector tail reads a
    tensor the tap or an output exposes."""
    rel = {"mode": "nmd", "hidden_layers": [_dense(1)]}
    return translated_cfg([_conv(width), {"name": "nmd", "config": {}}], [_dense(3)], pooling=pooling, masked=masked, rel=rel)


def pool_reference(prog, i: int, ids, taps):
    """POOL op ``i`` in float64 from the tapped output (and mask) of the conv in front of it -> (OpOut, positions); raises the
    tap's refusal where that conv stores nothing."""
    from oracle import ops
    op = prog.ops[i]
    st = ops.State(ops.program_rows(prog, ids))
    src = next(j for j in range(i - 1, -1, -1) if prog.ops[j].kind == ops.OP_CONV and prog.ops[j].out_buf == op.in_buf)
    st.act[op.in_buf] = taps.get(src)
    mk = taps.mask(i, op.in_mask)
    if mk is not None:
        st.mask[op.in_mask] = mk
    return ops.run_op(prog, i, st), st.act[op.in_buf].shape[1] * st.act[op.in_buf].shape[2]


def tail_checks(prog, ids, out: dict, taps, precision: str = "f32"):
    """The per-op loop of the vector tail (tests/test_gpu_fused_kernels.py part D): the unfused POOL from the tapped output and
    mask of the conv in front of it, every NMD finish from the tapped output of the conv whose last stage is its tap, every
    dense layer that reads ``embedding`` / ``nmd`` and writes ``prediction`` / ``reliability``, each in float64 from what the GPU
    produced (``taps``: ``get(op)`` / ``mask(op, slot)``; ``out``: the forward's outputs).  Yields (op index, what, result, ok);
    a store-free conv (the max pool fused into it) is skipped."""
    from jaeger_amd import _lib as L
    from oracle import ops
    for i, op in enumerate(prog.ops):
        if op.kind == ops.OP_POOL:
            try:
                ref, n_pos = pool_reference(prog, i, ids, taps)
            except L.JaegerHipError as exc:          # a store-free conv (fused max pool): tests/test_gpu_op_taps.py's case
                assert "store-free" in str(exc), str(exc)
                continue
            got = out["embedding"][:, op.vec_off:op.vec_off + op.cout]
            res, ok = (fc.check_vec(got, ref.out, ref.M, gamma_sum(n_pos, precision), rms_sum(n_pos, precision))
                       if op.arg == ops.POOL_AVG else fc.check_vec(got, ref.out, ref.M, 0.0, 2.0 ** -24))
            what = "pool"
        elif op.kind == ops.OP_NMD_FINAL:
            src = max(j for j in range(i) if prog.ops[j].kind == ops.OP_CONV
                      and prog.ops[j].stages[prog.ops[j].n_stages - 1].kind == ops.ST_NMD
                      and prog.ops[j].stages[prog.ops[j].n_stages - 1].arg == op.arg)
            st = ops.State(ops.program_rows(prog, ids))
            try:
                st.part[op.arg] = taps.get(src)         # (the tap is the conv's last stage: its stored output is what it saw)
            except L.JaegerHipError as exc:
                assert "store-free" in str(exc), str(exc)
                continue
            mk = taps.mask(i, op.in_mask)
            if mk is not None:
                st.mask[op.in_mask] = mk
            ref = ops.run_op(prog, i, st)
            n_pos = st.part[op.arg].shape[1] * st.part[op.arg].shape[2]
            got = out["nmd"][:, op.vec_off:op.vec_off + op.cout]
            res, ok = fc.check_vec(got, ref.out, ref.M, gamma_sum(n_pos, precision), rms_sum(n_pos, precision))
            what = "nmd finish"
        elif op.kind == ops.OP_DENSE and op.in_vec in (ops.VEC_EMBEDDING, ops.VEC_NMD) and op.out_vec in (ops.VEC_PREDICTION, ops.VEC_RELIABILITY):
            st = ops.State(ops.program_rows(prog, ids))
            src_name = "embedding" if op.in_vec == ops.VEC_EMBEDDING else "nmd"
            st.vec[op.in_vec] = out[src_name]
            ref = ops.run_op(prog, i, st).out
            w = np.abs(np.asarray(prog.blob[op.w_off:op.w_off + op.cin * op.cout], np.float64)).reshape(op.cin, op.cout)
            mag = np.abs(out[src_name][:, :op.cin].astype(np.float64)) @ w
            if op.b_off >= 0:
                mag = mag + np.abs(np.asarray(prog.blob[op.b_off:op.b_off + op.cout], np.float64))
            got = out["prediction" if op.out_vec == ops.VEC_PREDICTION else "reliability"][:, op.vec_off:op.vec_off + op.cout]
            res, ok = fc.check_vec(got, ref, mag, gamma_sum(op.cin + 1), rms_sum(op.cin + 1))
            what = "dense"
        else:
            continue
        yield i, what, res, ok


class OracleTaps:
    """The CPU tier's stand-in for the GPU tap: the float64 program run's tensors rounded to f32, as the GPU would store them."""

    def __init__(self, prog, ids):
        from oracle import ops
        self.prog, self.ids = prog, ids
        self.res = ops.run_program(prog, ids)

    def get(self, i):
        return self.res[i].out.astype(F)

    def mask(self, i, slot):
        from oracle import ops
        if slot in (ops.BUF_NONE, ops.BUF_IDS):
            return None
        j = max(j for j in range(i) if self.prog.ops[j].kind == ops.OP_MASK and self.prog.ops[j].out_mask == slot)
        return self.res[j].out


def emulate_pool(x: np.ndarray, mask, kind_avg: bool, mut: str | None = None) -> np.ndarray:
    """pool_kernel in f32: x (W, positions, C) f32, mask (W, positions) or None.  256 / (C / 4) groups of threads take the
    positions g, g + groups, ... in turn (masked ones skipped), thread group 0 adds the partial results in turn."""
    n_win, pos, c = x.shape
    groups = 256 // (c // 4)
    keep = np.ones((n_win, pos), bool) if mask is None else np.asarray(mask).reshape(n_win, pos) != 0
    parts, cnts = [], []
    for g in range(groups):
        acc = np.full((n_win, c), -np.inf if not kind_avg else 0.0, F)
        cnt = np.zeros(n_win, F)
        for p in range(g, pos, groups):
            k = keep[:, p]
            cnt = cnt + k.astype(F)
            acc = np.where(k[:, None], np.maximum(acc, x[:, p]) if not kind_avg else (acc + x[:, p]).astype(F), acc)
        parts.append(acc)
        cnts.append(cnt)
    acc, cnt = parts[0], cnts[0]
    for g in range(1, groups):
        acc = np.maximum(acc, parts[g]) if not kind_avg else (acc + parts[g]).astype(F)
        cnt = cnt + cnts[g]
    if not kind_avg:
        if mask is None:
            return acc
        r = np.where((cnt < pos)[:, None], np.maximum(acc, F(-1.0e9)), acc)
        return np.where((cnt <= 0)[:, None], F(0), r).astype(F)
    if mut == "pool averaging over all positions instead of the mask count":
        return (acc / F(pos)).astype(F)
    d = np.maximum(cnt, F(1e-7)) if mask is not None else np.full(n_win, pos, F)
    return (acc / d[:, None]).astype(F)


def emulate_nmd_final(x: np.ndarray, mask, mm: np.ndarray, eps: float, mut: str | None = None, frames: int = 6) -> np.ndarray:
    """The tap sums and nmd_final_kernel in f32: x (W, frames x L, C); one partial row per frame (rows this short are one tile),
    the masked positions of a frame added in turn; the finish adds the partial rows in turn, / (count + eps), - moving mean."""
    n_win, pos, c = x.shape
    keep = np.ones((n_win, pos), bool) if mask is None else np.asarray(mask).reshape(n_win, pos) != 0
    per = pos // frames
    acc = np.zeros((n_win, c), F)
    for f in range(frames):
        part = np.zeros((n_win, c), F)
        for p in range(f * per, (f + 1) * per):
            part = np.where(keep[:, p, None], (part + x[:, p]).astype(F), part)
        acc = (acc + part).astype(F)
    cnt = keep.sum(axis=1).astype(F)
    e = F(0) if mut == "NMD finish dividing without eps" else F(eps)
    d = (cnt + e).astype(F) if mask is not None else np.full(n_win, pos, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((acc / d[:, None]).astype(F) - mm.astype(F)).astype(F)


# ---- 3. VECMAX --------------------------------------------------------------------------------------------------------------
#: name -> (taps, target_dim, projection activation)
VECMAX_CASES = {"two taps t=10": (2, 10, None), "two taps t=10 gelu": (2, 10, "gelu"), "three taps t=10": (3, 10, None),
                "three taps t=10 tanh": (3, 10, "tanh"), "two taps t=24": (2, 24, None), "two taps t=24 sigmoid": (2, 24, "sigmoid"),
                "three taps t=24": (3, 24, None), "three taps t=24 relu": (3, 24, "relu")}


def vecmax_family(name: str) -> Family:
    """``max``: NMDMerge(mode max, target_dim) over two or three taps (two convs at the most: conv 24, nmd, gelu, nmd [, conv 40,
    nmd]); ``concat``: the same representation learner with the taps side by side as ``nmd``."""
    taps, target, act = VECMAX_CASES[name]
    tap = {"name": "nmd", "config": {}}
    rep = [_conv(24), tap, {"name": "gelu"}, tap] + ([_conv(40), tap] if taps == 3 else [])
    merge = {"mode": "max", "target_dim": target}
    if act is not None:
        merge["projection_kwargs"] = {"activation": act}
    cfgs = {"max": translated_cfg(rep, [_dense(3)], rel={"mode": "nmd", "merge": merge, "hidden_layers": [_dense(1)]}),
            "concat": translated_cfg(rep, [_dense(3)], rel={"mode": "nmd", "merge": {"mode": "concat"},
                                                              "hidden_layers": _at(1, _dense(1))})}
    return Family(cfgs)


def vecmax_ops(prog) -> tuple:
    """(index of the block-diagonal dense op, index of the VECMAX op behind it)."""
    from oracle import ops
    v = next(i for i, op in enumerate(prog.ops) if op.kind == ops.OP_VECMAX)
    d = max(i for i in range(v) if prog.ops[i].kind == ops.OP_DENSE and prog.ops[i].out_vec == prog.ops[v].in_vec)
    return d, v


def vecmax_reference(prog, raw: np.ndarray):
    """The block-diagonal dense in float64 from the raw tap vectors, then the maximum over the groups -> (ref, M, gamma, rms):
    |max a - max b| <= max |a - b|, so the dense layer's bound carries over with M = the largest of the groups' M."""
    d, v = vecmax_ops(prog)
    ref, mag, gamma, rms = dense_reference(prog, d, raw)
    k, t = prog.ops[v].k, prog.ops[v].cout
    return ref.reshape(len(raw), k, t).max(axis=1), mag.reshape(len(raw), k, t).max(axis=1), gamma, rms


def emulate_vecmax(prog, raw: np.ndarray, chunk: int = 0, mut: str | None = None) -> np.ndarray:
    d, v = vecmax_ops(prog)
    blocks = emulate_dense(prog, d, raw, chunk)
    k, t = prog.ops[v].k, prog.ops[v].cout
    stride = (t + 3) & ~3 if mut == "vecmax striding groups by the padded width" else t
    pitch = (k * t + 3) & ~3
    flat = np.zeros((len(raw), pitch), F)
    flat[:, :k * t] = blocks
    flat = np.concatenate([flat.ravel(), np.zeros(k * stride + t, F)])          # (a read past the last row: zeros)
    at = np.arange(len(raw))[:, None] * pitch + np.arange(t)[None, :]
    m = flat[at]
    for g in range(1, k):
        x = flat[at + g * stride]
        m = np.where((x > m) | (x != x), x, m)
    return m


# ---- 4. OODSIG ----------------------------------------------------------------------------------------------------------------
SIGNALS = ["max_prob", "entropy", "energy", "margin", "nmd_norm"]
#: name -> (classes, nmd width, signals)
OOD_CASES = {"3 classes nmd 10 all five": (3, 10, list(SIGNALS)),
             "7 classes nmd 8 all five reversed": (7, 8, ["nmd_norm", "margin", "energy", "entropy", "max_prob"]),
             "2 classes nmd 10 margin alone": (2, 10, ["margin"]),
             "3 classes nmd 8 three signals": (3, 8, ["energy", "nmd_norm", "max_prob"])}
OOD_FIRST_PLANTED = 50          # ids 1 .. 49 are the random windows' codons; ids from 50 up are the planted rows


def planted_logits(n_cls: int) -> dict:
    """name -> the logits of one constant-id window.  "near +-80": an f32 sum of exp(logit) is still in range there, so the rows
    that tell a missing max shift are the two at the ends of exp's f32 range (three times e^88.5 overflows, e^-100 is subnormal)."""
    k = n_cls
    ramp = np.arange(k) / 4.0
    rows = {"two equal maxima": np.r_[2.0, 2.0, -ramp[:k - 2] - 1.0][:k],
            "all classes equal": np.full(k, 0.75),
            "the maximum first": np.r_[3.0, 1.0 - ramp[:k - 1]],
            "the maximum last": np.r_[1.0 - ramp[:k - 1], 3.0],
            "one logit 60 above the rest": np.r_[-0.5 * np.ones(k - 1), 59.5],
            "logits near +80": 80.0 + ramp - 0.5,
            "logits near -80": -80.0 - ramp + 0.25,
            "logits at +88.5": 88.5 - ramp / 8.0,
            "logits at -100": -100.0 + ramp / 2.0}
    for v in rows.values():
        assert v.shape == (k,) and (v.astype(np.float32) == v).all()
    return rows


def ood_family(name: str) -> tuple:
    """A model whose logits are rows of its embedding table: embedding 8 -> a 3-tap conv whose middle tap is the identity (no
    bias: its output IS the embedding row at every valid position) -> max pool -> the first ``n_cls`` channels as logits (an
    identity classifier) -> an identity reliability head: ``reliability`` = [nmd | signals].  nmd 8: the one tap; nmd 10: two
    taps through NMDMerge(max, target_dim 10), which puts the signal block at an offset that is no multiple of 4.
    Returns (family, ids (13 random windows + the planted ones), names of the planted windows)."""
    n_cls, nmd_dim, signals = OOD_CASES[name]
    tap = {"name": "nmd", "config": {}}
    rep = [_conv(8, bias=False), tap] + ([tap] if nmd_dim != 8 else [])          # (two taps of the same tensor, two projections)
    rel = {"mode": "nmd_plus_signals", "signals": list(signals),
           "hidden_layers": [_dense(nmd_dim + len(signals), None, False)]}
    if nmd_dim != 8:
        rel["merge"] = {"mode": "max", "target_dim": nmd_dim}
    cfg = translated_cfg(rep, [_dense(n_cls, None, False)], e=8, rel=rel)
    rng = np.random.Generator(np.random.PCG64(97))
    table = rng.normal(0.0, 1.5, (65, 8)).astype(np.float32)
    planted = planted_logits(n_cls)
    for q, v in enumerate(planted.values()):
        table[OOD_FIRST_PLANTED + q, :n_cls] = v
    kernel = np.zeros((3, 8, 8), np.float32)
    kernel[1] = np.eye(8, dtype=np.float32)
    over = {"embedding/embeddings": table, "rep/0/kernel": kernel, "classifier/0/kernel": np.eye(8, dtype=np.float32)[:, :n_cls].copy(),
            "reliability/0/kernel": np.eye(nmd_dim + len(signals), dtype=np.float32)}
    fam = Family({"ood": cfg}, over)
    ids = np.concatenate([oc.edge_ids(CODONS, n_win=ROWS, vocab=OOD_FIRST_PLANTED),
                          np.stack([np.full((6, CODONS), OOD_FIRST_PLANTED + q, np.uint8) for q in range(len(planted))])])
    return fam, ids, list(planted)


def ood_op(prog) -> int:
    from oracle import ops
    return next(i for i, op in enumerate(prog.ops) if op.kind == ops.OP_OODSIG)


def ood_reference(prog, logits: np.ndarray, nmd: np.ndarray):
    """oracle/ops.py's ``_signals`` on the given logits and nmd -> (ref, M): M = 1 + |signal| for the four that come from the
    softmax (probabilities are held to absolute errors), the norm itself for ``nmd_norm`` (a sum of squares: relative)."""
    from oracle import ops
    i = ood_op(prog)
    op = prog.ops[i]
    st = ops.State(np.zeros((len(logits), 1, 1), np.uint8))
    st.vec[op.in_vec] = np.asarray(logits, np.float64)
    st.vec[op.k] = np.asarray(nmd, np.float64)
    ref = ops.run_op(prog, i, st).out
    mag = 1.0 + np.abs(ref)
    for j in range(op.cout):
        if (op.arg >> (4 * j)) & 15 == 5:
            mag[:, j] = np.abs(ref[:, j])
    return ref, mag


def emulate_oodsig(prog, logits: np.ndarray, nmd: np.ndarray, mut: str | None = None) -> np.ndarray:
    """oodsig_kernel in f32 in the kernel's order -> the row [nmd | signals] an identity reliability head shows."""
    i = ood_op(prog)
    op = prog.ops[i]
    n_cls, nmd_w, eps, order = op.cin, op.stride, F(op.f0), op.arg
    lg = np.asarray(logits, F)[:, :n_cls]
    nm = np.asarray(nmd, F)[:, :nmd_w]
    n = len(lg)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        mx = lg.max(axis=1)
        shift = np.zeros(n, F) if mut == "energy without the max shift" else mx
        se = np.zeros(n, F)
        for c in range(n_cls):
            se = (se + np.exp((lg[:, c] - mx).astype(F)).astype(F)).astype(F)
        p1, p2, ent = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        for c in range(n_cls):
            p = (np.exp((lg[:, c] - mx).astype(F)).astype(F) / se).astype(F)
            first = p > p1
            second = ~first & (p > p2) & (mut != "margin without the else-if branch")
            p2 = np.where(first, p1, np.where(second, p, p2))
            p1 = np.where(first, p, p1)
            sp = np.maximum(p, eps)
            ent = (ent - (sp * np.log(sp).astype(F)).astype(F)).astype(F)
        if mut == "energy without the max shift":
            s0 = np.zeros(n, F)
            for c in range(n_cls):
                s0 = (s0 + np.exp((lg[:, c] - shift).astype(F)).astype(F)).astype(F)
            energy = np.log(s0).astype(F)
        else:
            energy = (mx + np.log(se).astype(F)).astype(F)
        out_off = (nmd_w + 3) & ~3 if mut == "signal block written at the offset rounded up to 4" else nmd_w
        row = np.zeros((n, out_off + op.cout + 4), F)
        row[:, :nmd_w] = nm
        for j in range(op.cout):
            code = (order >> (4 * j)) & 15
            if code == 5:
                w = (nmd_w + 3) & ~3 if mut == "nmd_norm over the padded width" else nmd_w
                ss = np.zeros(n, F)
                for c in range(w):
                    ss = _fma(ss, row[:, c], row[:, c])        # (beyond the nmd: whatever the slot holds there by now)
                v = np.sqrt(ss).astype(F)
            else:
                v = {1: p1, 2: ent, 3: energy, 4: (p1 - p2).astype(F)}[code]
            row[:, out_off + j] = v
    return row[:, :nmd_w + op.cout]


OOD_MUTATIONS = ("signal block written at the offset rounded up to 4", "margin without the else-if branch",
                 "energy without the max shift", "nmd_norm over the padded width")


# ---- 5. strand merge ----------------------------------------------------------------------------------------------------------
STRAND_BASES = 60
STRAND_WINDOWS = (5, 3)          # 10 strand rows: dense_tiled with a tail of 2; 6 rows: the plain kernel


def strand_family() -> Family:
    """The dvf500 layout at 60 bases - conv1d 500 x 10, relu, max1d; dropout, dense 500 relu, dropout, dense 3, merge - with
    every merge method, the head cut behind the 500 -> 500 layer (``prefix``: merge concat shows its rows per strand) and an
    identity head (``identity``: merge concat shows the pooled vector per strand)."""
    from conftest import load_model_cfg
    base = copy.deepcopy(load_model_cfg("dvf500"))
    base["string_processor"]["crop_size"] = STRAND_BASES

    def with_head(layers):
        cfg = copy.deepcopy(base)
        cfg["classifier"]["branch"]["hidden_layers"] = layers
        return cfg
    head = base["classifier"]["branch"]["hidden_layers"]
    assert [ly["name"] for ly in head] == ["dropout", "dense", "relu", "dropout", "dense", "merge"]

    def merge(m):
        return {"name": "merge", "config": {"method": m}}
    cfgs = {m: with_head(copy.deepcopy(head[:-1]) + [merge(m)]) for m in ("concat", "average", "sum", "max")}
    cfgs["prefix"] = with_head(copy.deepcopy(head[:3]) + [merge("concat")])
    cfgs["identity"] = with_head(_at(7, _dense(500, None, False)) + [merge("concat")])
    return Family(cfgs, {"classifier/7/kernel": np.eye(500, dtype=np.float32)}, strands=True)


def strand_expected(kind: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """What a merge of two strand rows must be, bit for bit: with two operands the f32 result is unique."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return {"max": np.maximum(a, b), "sum": a + b, "average": (a + b) / F(2)}[kind]


def emulate_strand_merge(a: np.ndarray, b: np.ndarray, kind: str, mut: str | None = None) -> np.ndarray:
    """strand_merge_kernel on two strand rows as its source states it: acc = the first row, fmaxf or + the second, / strands."""
    acc, b = np.asarray(a, F), np.asarray(b, F)
    as_max = kind == "max" or (kind == "sum" and mut == "strand sum taken as max")
    acc = np.maximum(acc, b) if as_max else (acc + b).astype(F)
    return (acc / F(2)).astype(F) if kind == "average" else acc


def distance(res, rms_bound: float) -> float:
    """How far beyond the check a result sits: the larger of err / bound and RMS / its bound; not finite = infinitely far."""
    if not (math.isfinite(res.worst) and math.isfinite(res.rms)):
        return math.inf
    return max(res.worst, res.rms / rms_bound)
