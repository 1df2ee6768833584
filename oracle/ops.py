"""Oracle: float64 interpreter of the compiled op program (TEST INFRASTRUCTURE, see oracle/__init__.py).

A restatement of the op semantics ``include/jaeger_hip.h`` documents, evaluated in float64 numpy on a compiled
``Program`` (its ``ops`` and its f32 weight ``blob``) - the product never imports it.  Two uses:

* ``run_program`` chains every op from the id tensor: it must compute what ``oracle.forward`` computes in float64, up to
  the rounding of the parameters the program stores in f32 (``tests/test_op_reference.py``) - this pins
  ``jaeger_amd/program.py`` on the CPU.
* ``run_op`` evaluates ONE op from given inputs (the tensors the GPU tap read back, ``tests/test_gpu_op_taps.py``), so that a
  kernel's output is compared with an exact evaluation of that op alone.

Tensors are laid out like the engine's: activations (rows, frames, L, C), masks (rows, frames, L) (0 / 1), vectors
(rows, width); rows = program rows (windows, or windows x strands).  A conv's result also carries its magnitude ``M``
(a pool's or an NMD finish's: the same pool / mean of its input's magnitude under the same mask, plus ``|moving mean|``):
the same linear part evaluated on ``|x * mask|`` and ``|W|``, plus ``|bias|``, through ``|BN scale|`` (plus ``|scale * mean|
+ |beta|``), plus ``|residual|``, times the Lipschitz constant of every activation on the way (plus ``|f(0)|``: the sigmoid's
1 / 2) - the scale of what the
kernel summed, which the error bounds are written in.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

# the enums of include/jaeger_hip.h (restated: the checker does not read them from the code under test)
OP_CONV, OP_MASK, OP_POOL, OP_DENSE, OP_ELTWISE, OP_NMD_FINAL, OP_OODSIG, OP_MAXPOOL1D, OP_FRAMESUM, OP_STRANDS, OP_EMBED, \
    OP_VECMAX = range(1, 13)
ST_BIAS, ST_BN, ST_DYT, ST_ADD, ST_ACT, ST_NMD, ST_MASKMUL, ST_LN = range(1, 9)
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_RELU, ACT_TANH, ACT_SIGMOID = range(6)
MASK_ANY, MASK_MAJORITY, MASK_STRICT = range(3)
PAD_VALID, PAD_SAME = 0, 1
POOL_MAX, POOL_AVG, POOL_MAX_NOMASK = 0, 1, 2
MERGE_AVERAGE, MERGE_SUM, MERGE_MAX, MERGE_CONCAT = range(4)
BUF_NONE, BUF_IDS = -1, -2
VEC_EMBEDDING, VEC_NMD, VEC_PREDICTION, VEC_RELIABILITY = range(4)

#: Lipschitz constant of each activation (max |f'|): tanh-GELU and erf-GELU 1.13, sigmoid 1 / 4
LIPSCHITZ = {ACT_NONE: 1.0, ACT_GELU_TANH: 1.13, ACT_GELU_ERF: 1.13, ACT_RELU: 1.0, ACT_TANH: 1.0, ACT_SIGMOID: 0.25}


def act(kind: int, x: np.ndarray) -> np.ndarray:
    if kind == ACT_NONE:
        return x
    if kind == ACT_GELU_TANH:
        return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * (x * x * x))))
    if kind == ACT_GELU_ERF:
        return 0.5 * x * torch.erfc(torch.from_numpy(-x * 0.7071067811865476)).numpy()
    if kind == ACT_RELU:
        return np.maximum(x, 0.0)
    if kind == ACT_TANH:
        return np.tanh(x)
    if kind == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-x))
    raise ValueError(f"activation {kind}")


def conv_geometry(l_in: int, k: int, stride: int, dil: int, padding: int) -> tuple[int, int]:
    """(L_out, pad_left): TF SAME (pad_left = total // 2) or VALID - jg_model.hip conv_geometry."""
    if padding == PAD_SAME:
        lo = -(-l_in // stride)
        total = max((lo - 1) * stride + (k - 1) * dil + 1 - l_in, 0)
        return lo, total // 2
    span = dil * (k - 1) + 1
    return ((l_in - span) // stride + 1 if l_in >= span else 0), 0


def shifted_sum(x: np.ndarray, w: np.ndarray, stride: int, dil: int, pad_left: int, l_out: int) -> np.ndarray:
    """y[..., m, :] = sum_t x[..., m s + t d - pad_left, :] @ w[t] with zeros outside the row.  x (..., L, Cin), w (k, Cin, Cout)."""
    k = w.shape[0]
    l_in = x.shape[-2]
    y = np.zeros(x.shape[:-2] + (l_out, w.shape[2]))
    for t in range(k):
        # outputs m with 0 <= m s + t d - pad_left < l_in: a contiguous range (slices and one 2-D product per tap: index
        # arrays and a batched product run ten times slower on tensors of this size; torch's float64 product: numpy's
        # BLAS takes milliseconds to start its threads for a product this small)
        off = t * dil - pad_left
        m0 = max(0, -(off // stride))
        m1 = min(l_out, (l_in - 1 - off) // stride + 1)
        if m1 > m0:
            xs = x[..., m0 * stride + off:(m1 - 1) * stride + off + 1:stride, :]
            prod = torch.from_numpy(xs.reshape(-1, xs.shape[-1])) @ torch.from_numpy(np.ascontiguousarray(w[t]))
            y[..., m0:m1, :] += prod.numpy().reshape(xs.shape[:-1] + (w.shape[2],))
    return y


@dataclass
class OpOut:
    out: np.ndarray                       # activation (rows, frames, L, C), mask (rows, frames, L) u8, or vector (rows, C)
    M: np.ndarray | None = None           # magnitude of a conv / element-wise result (same shape as out)
    mask: np.ndarray | None = None        # EMBED: the mask it writes
    taps: dict = field(default_factory=dict)   # NMD partial slot -> the tensor the ST_NMD stage saw
    taps_M: dict = field(default_factory=dict)  # NMD partial slot -> that tensor's magnitude


@dataclass
class State:
    """What the ops read: the id tensor (rows, frames, L) and the slots the earlier ops wrote."""
    ids: np.ndarray
    act: dict = field(default_factory=dict)
    mask: dict = field(default_factory=dict)
    part: dict = field(default_factory=dict)
    vec: dict = field(default_factory=dict)
    M: dict = field(default_factory=dict)     # slot -> magnitude of an activation that is itself a reference (not a readback)
    part_M: dict = field(default_factory=dict)   # NMD partial slot -> magnitude of the tapped tensor (default: its absolute value)


def _blob(program, off: int, n: int) -> np.ndarray:
    return np.asarray(program.blob[off:off + n], np.float64)


def _mask_of(state: State, slot: int):
    if slot == BUF_NONE:
        return None
    if slot == BUF_IDS:
        return (state.ids != 0).astype(np.float64)
    return np.asarray(state.mask[slot], np.float64)


def conv_weights(program, op) -> np.ndarray:
    cin_pad, cout_pad = (op.cin + 1) & ~1, (op.cout + 31) // 32 * 32
    return _blob(program, op.w_off, op.k * cin_pad * cout_pad).reshape(op.k, cin_pad, cout_pad)[:, :op.cin, :op.cout]


def conv_input(program, op, state: State) -> np.ndarray:
    """The conv's input times its input mask (the kernels multiply on the way in)."""
    if op.in_buf == BUF_IDS:
        table = _blob(program, op.b_off, program.vocab * op.cin).reshape(program.vocab, op.cin)
        x = table[state.ids.astype(np.int64)]
    else:
        x = np.asarray(state.act[op.in_buf], np.float64)
    m = _mask_of(state, op.in_mask)
    return x if m is None else x * m[..., None]


def _stages(program, op, v: np.ndarray, M: np.ndarray, state: State, first: int = 0):
    c = op.cout
    out_mask = _mask_of(state, op.out_mask)
    taps, taps_m = {}, {}
    for s in range(first, op.n_stages):
        st = op.stages[s]
        if st.kind == ST_BIAS:
            b = _blob(program, st.p0, c)
            v, M = v + b, M + np.abs(b)
        elif st.kind == ST_BN:
            mu, inv, g, beta = (_blob(program, p, c) for p in (st.p0, st.p1, st.p2, st.p3))
            v = g * ((v - mu) * inv) + beta
            M = np.abs(g * inv) * (M + np.abs(mu)) + np.abs(beta)
        elif st.kind == ST_DYT:
            g, beta = _blob(program, st.p2, c), _blob(program, st.p3, c)
            alpha = float(np.float32(st.f0))
            v = np.tanh(alpha * v) * g + beta
            M = np.abs(alpha * g) * M + np.abs(beta)
            if st.arg and out_mask is not None:
                v, M = v * out_mask[..., None], M * out_mask[..., None]
        elif st.kind == ST_ADD:
            r = np.asarray(state.act[st.arg], np.float64)
            v, M = v + r, M + state.M.get(st.arg, np.abs(r))
        elif st.kind == ST_ACT:
            v, M = act(st.arg, v), M * LIPSCHITZ[st.arg] + (0.5 if st.arg == ACT_SIGMOID else 0.0)    # (+ |f(0)|)
        elif st.kind == ST_NMD:
            taps[st.arg] = v.copy()
            taps_m[st.arg] = M.copy()
        elif st.kind == ST_MASKMUL:
            if out_mask is not None:
                v, M = v * out_mask[..., None], M * out_mask[..., None]
        elif st.kind == ST_LN:
            g, beta = _blob(program, st.p2, c), _blob(program, st.p3, c)
            eps = float(np.float32(st.f0))
            if st.arg and out_mask is not None:
                v, M = v * out_mask[..., None], M * out_mask[..., None]
            mean = v.mean(axis=-1, keepdims=True)
            rs = 1.0 / np.sqrt(((v - mean) ** 2).mean(axis=-1, keepdims=True) + eps)
            M = np.abs(g) * (np.abs(v) + np.abs(mean)) * rs + np.abs(beta)
            v = (v - mean) * rs * g + beta
            if st.arg and out_mask is not None:
                v, M = v * out_mask[..., None], M * out_mask[..., None]
        else:
            raise ValueError(f"stage kind {st.kind}")
    return v, M, (taps, taps_m)


def mask_rule(m_in: np.ndarray, k: int, stride: int, dil: int, padding: int, mode: int) -> np.ndarray:
    """JG_OP_MASK (layers.py:1226-1255): the count of valid inputs under the window, then any / majority / strict."""
    lo, pl = conv_geometry(m_in.shape[-1], k, stride, dil, padding)
    cnt = shifted_sum(m_in[..., None].astype(np.float64), np.ones((k, 1, 1)), stride, dil, pl, lo)[..., 0]
    if mode == MASK_ANY:
        om = cnt > 0
    elif mode == MASK_MAJORITY:
        om = cnt >= (k + 1) // 2
    else:
        om = cnt == k
    return om.astype(np.uint8)


def _signals(logits, nmd, order: int, n: int, eps: float) -> np.ndarray:
    z = logits - logits.max(axis=-1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(axis=-1, keepdims=True)
    cols = []
    for j in range(n):
        code = (order >> (4 * j)) & 15
        if code == 1:
            cols.append(p.max(axis=-1))
        elif code == 2:
            sp = np.maximum(p, eps)
            cols.append(-(sp * np.log(sp)).sum(axis=-1))
        elif code == 3:
            mx = logits.max(axis=-1)
            cols.append(mx + np.log(np.exp(logits - mx[:, None]).sum(axis=-1)))
        elif code == 4:
            s = np.sort(p, axis=-1)
            cols.append(s[:, -1] - s[:, -2])
        elif code == 5:
            cols.append(np.sqrt((nmd ** 2).sum(axis=-1)))
        else:
            raise ValueError(f"signal code {code}")
    return np.stack(cols, axis=-1)


def run_op(program, i: int, inputs: State) -> OpOut:
    """Op ``i`` of ``program`` in float64 from the slots of ``inputs`` (nothing in ``inputs`` is modified)."""
    op = program.ops[i]
    st = inputs
    if op.kind == OP_CONV:
        x = conv_input(program, op, st)
        w = conv_weights(program, op)
        lo, pl = conv_geometry(x.shape[-2], op.k, op.stride, op.dilation, op.padding)
        y = shifted_sum(x, w, op.stride, op.dilation, pl, lo)
        ax = np.abs(x)
        if op.in_buf in st.M:                 # a reference input: its own error scales with its magnitude
            m = _mask_of(st, op.in_mask)
            ax = st.M[op.in_buf] if m is None else st.M[op.in_buf] * m[..., None]
        M = shifted_sum(ax, np.abs(w), op.stride, op.dilation, pl, lo)
        y, M, (taps, taps_m) = _stages(program, op, y, M, st)
        return OpOut(y, M, taps=taps, taps_M=taps_m)
    if op.kind == OP_ELTWISE:
        x = np.asarray(st.act[op.in_buf], np.float64)
        y, M, (taps, taps_m) = _stages(program, op, x, np.abs(x), st)
        return OpOut(y, M, taps=taps, taps_M=taps_m)
    if op.kind == OP_MASK:
        m = _mask_of(st, op.in_mask)
        return OpOut(mask_rule(m, op.k, op.stride, op.dilation, op.padding, op.mask_mode))
    if op.kind == OP_EMBED:
        ids = st.ids.astype(np.int64)
        x = _blob(program, op.b_off, program.vocab * op.cout).reshape(program.vocab, op.cout)[ids]
        if op.w_off >= 0:
            x = x + _blob(program, op.w_off, op.k * op.cout).reshape(op.k, op.cout)[:ids.shape[-1]]
        return OpOut(x, np.abs(x), mask=(ids != 0).astype(np.uint8))
    if op.kind == OP_MAXPOOL1D:
        x = np.asarray(st.act[op.in_buf], np.float64)
        lo = x.shape[-2] // 2
        return OpOut(np.maximum(x[..., 0:2 * lo:2, :], x[..., 1:2 * lo:2, :]))
    if op.kind == OP_FRAMESUM:
        x = np.asarray(st.act[op.in_buf], np.float64)
        return OpOut(x.sum(axis=1, keepdims=True), np.abs(x).sum(axis=1, keepdims=True))
    if op.kind == OP_POOL:
        # M: the same pool of the input's magnitude under the same mask (|max a - max b| <= max |a - b|)
        x = np.asarray(st.act[op.in_buf], np.float64)
        ax = np.asarray(st.M.get(op.in_buf, np.abs(x)), np.float64)
        x = x.reshape(x.shape[0], -1, x.shape[-1])
        ax = ax.reshape(x.shape)
        m = _mask_of(st, op.in_mask)
        if m is None or op.arg == POOL_MAX_NOMASK:
            return OpOut(x.mean(axis=1), ax.mean(axis=1)) if op.arg == POOL_AVG else OpOut(x.max(axis=1), ax.max(axis=1))
        m = m.reshape(m.shape[0], -1, 1)
        if op.arg == POOL_AVG:
            cnt = np.maximum(m.sum(axis=1), 1e-7)
            return OpOut((x * m).sum(axis=1) / cnt, (ax * m).sum(axis=1) / cnt)
        some = m.max(axis=1) > 0
        pooled = np.where(m > 0, x, -1.0e9).max(axis=1)
        return OpOut(np.where(some, pooled, 0.0), np.where(some, (ax * m).max(axis=1), 0.0))
    if op.kind == OP_NMD_FINAL:
        part = np.asarray(st.part[op.arg], np.float64)
        apart = np.asarray(st.part_M.get(op.arg, np.abs(part)), np.float64)
        part = part.reshape(part.shape[0], -1, part.shape[-1])
        apart = apart.reshape(part.shape)
        mm = _blob(program, op.b_off, op.cout)
        m = _mask_of(st, op.in_mask)
        if m is None:
            return OpOut(part.mean(axis=1) - mm, apart.mean(axis=1) + np.abs(mm))
        m = m.reshape(m.shape[0], -1, 1)
        cnt = m.sum(axis=1) + float(np.float32(op.f0))
        return OpOut((part * m).sum(axis=1) / cnt - mm, (apart * m).sum(axis=1) / cnt + np.abs(mm))
    if op.kind == OP_DENSE:
        v = np.asarray(st.vec[op.in_vec], np.float64)[:, :op.cin]
        y = v @ _blob(program, op.w_off, op.cin * op.cout).reshape(op.cin, op.cout)
        if op.b_off >= 0:
            y = y + _blob(program, op.b_off, op.cout)
        return OpOut(act(op.arg, y))
    if op.kind == OP_OODSIG:
        logits = np.asarray(st.vec[op.in_vec], np.float64)[:, :op.cin]
        nmd = np.asarray(st.vec[op.k], np.float64)[:, :op.stride]
        return OpOut(_signals(logits, nmd, op.arg, op.cout, float(np.float32(op.f0))))
    if op.kind == OP_VECMAX:
        v = np.asarray(st.vec[op.in_vec], np.float64)[:, :op.k * op.cout]
        return OpOut(v.reshape(v.shape[0], op.k, op.cout).max(axis=1))
    raise ValueError(f"op {i}: kind {op.kind} has no tensor or vector result")


def _put_vec(state: State, slot: int, off: int, v: np.ndarray) -> None:
    cur = state.vec.get(slot)
    width = off + v.shape[1]
    if cur is None:
        cur = np.zeros((v.shape[0], width))
    elif cur.shape[1] < width:
        cur = np.concatenate([cur, np.zeros((cur.shape[0], width - cur.shape[1]))], axis=1)
    cur = cur.copy()
    cur[:, off:width] = v
    state.vec[slot] = cur


def program_rows(program, ids: np.ndarray) -> np.ndarray:
    """ids (W, 6, L) -> program rows (W, 6, L); a two-strand model's (W, strands, L) -> (W x strands, 1, L)."""
    ids = np.asarray(ids)
    if getattr(program, "strands", 1) > 1:
        return ids.reshape(-1, 1, ids.shape[-1])
    return ids


def apply(program, i: int, state: State, res: OpOut) -> None:
    """Write op ``i``'s result into the slots it owns."""
    op = program.ops[i]
    if op.kind == OP_MASK:
        state.mask[op.out_mask] = res.out
    elif op.kind in (OP_CONV, OP_ELTWISE, OP_MAXPOOL1D, OP_FRAMESUM, OP_EMBED):
        state.act[op.out_buf] = res.out
        if res.mask is not None:
            state.mask[op.out_mask] = res.mask
        state.part.update(res.taps)
        state.part_M.update(res.taps_M)
    elif op.kind in (OP_POOL, OP_NMD_FINAL, OP_DENSE, OP_OODSIG, OP_VECMAX):
        _put_vec(state, op.out_vec, op.vec_off, res.out)


def run_program(program, ids: np.ndarray, keep=None) -> dict:
    """{op index: OpOut} of every op that stores a tensor or a vector, chained from the id tensor.  ``keep``: indices to
    return (default all); the final vector slots are under the key ``"vec"``."""
    state = State(program_rows(program, ids))
    results = {}
    for i, op in enumerate(program.ops):
        if op.kind == OP_STRANDS:
            continue
        res = run_op(program, i, state)
        apply(program, i, state, res)
        if keep is None or i in keep:
            results[i] = res
    results["vec"] = state.vec
    return results


def outputs(program, ids: np.ndarray) -> dict:
    """The model's outputs (prediction, reliability, embedding, nmd) from ``run_program``'s vector slots, per window."""
    vec = run_program(program, ids, keep=())["vec"]
    n_win = np.asarray(ids).shape[0]
    widths = {"prediction": program.n_classes, "embedding": program.embedding_dim}
    if program.has_reliability:
        widths["reliability"] = 1
    if program.nmd_dim:
        widths["nmd"] = program.nmd_dim
    slot = {"prediction": VEC_PREDICTION, "reliability": VEC_RELIABILITY, "embedding": VEC_EMBEDDING, "nmd": VEC_NMD}
    out = {}
    for name, wd in widths.items():
        if slot[name] not in vec:
            continue
        v = vec[slot[name]]
        wd = v.shape[1] if name == "reliability" else wd
        v = v[:, :wd]
        strands = getattr(program, "strands", 1)
        if strands > 1:
            v = v.reshape(n_win, strands, wd)
            kind = next(o.arg for o in program.ops if o.kind == OP_STRANDS) if name == "prediction" else MERGE_AVERAGE
            v = {MERGE_AVERAGE: lambda a: a.mean(axis=1), MERGE_SUM: lambda a: a.sum(axis=1),
                 MERGE_MAX: lambda a: a.max(axis=1), MERGE_CONCAT: lambda a: a.reshape(n_win, -1)}[kind](v)
        out[name] = v
    return out
