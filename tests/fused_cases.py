"""Shared cases of the fused whole-row kernels' checks (tests/test_fused_reference.py on the CPU, tests/test_gpu_fused_kernels.py
on the GPU): ``small_net_kernel`` (jg_small.hip: ids -> pooled sums of the 32-channel 500-bp family in one launch) and the two
table-net strand kernels (``tab_mfma_kernel`` in jg_tabnet.hip, ``tab_conv_pool_kernel`` in jg_kernels.hip).  None of them
stores a tensor, so what they are held to is what they emit - the pooled ``embedding`` and, for the small kernel, the NMD taps
(the masked channel mean behind every layer that ends in an ``nmd`` stage) - against the float64 op interpreter
(oracle/ops.py) chained from the ids, which are exact: there is no upstream error to discount.

Here: the model variants (and which compiled epilogue of jg_small.hip each is there for), the seeded inputs (edge rows, probe
windows whose ids are valid in a dozen positions only - so each position of each layer is seen almost alone -, multi-row sets
that take every wave round its row loop three times or more), the check, and numpy emulations of the kernels' arithmetic with
the mutations the check must catch.

The check.  An observable (a pooled vector or a tap mean) with float64 reference ``ref`` and magnitude ``M`` (oracle/ops.py: the
same pool / mean of the producing layer's magnitude under the same mask) obeys, element by element,

    |got - ref| <= GAMMA * M + 2^-21 |ref| + 2^-24        and        RMS(|got - ref| / M) <= RMS_BOUND

The layers are chained, so ``M`` is the magnitude of the LAST layer in front of the observable and GAMMA covers what the
layers before it hand down; that is why GAMMA here is wider than tests/op_cases.py's per-op constant.

Constants (tests/test_fused_reference.py::test_bounds_sit_between_emulation_and_mutations re-measures every margin on each
run and prints the pair that catches each mutation):

    small_net_kernel (31 variants x 7 input sets; mutations tried on chain4, mix_c, nmdmerge500, mix_d_max, baseline500_max,
    baseline500_nomask in this order, the search stops at the first pair that catches a mutation by 8x: what the test prints)
    GAMMA     = 2^-19 (1.9e-6)   largest emulated err / M 3.1e-7, err / bound 0.15 (mix_b_max, probe windows l = 70, embedding)
                                                                                                              -> 6.1x above it
                                 smallest mutation: the shortcut's lo half dropped, 13.7x the bound (mix_c, probe windows,
                                 nmd: err / M 2.7e-5); hi_x lo_w dropped in one layer 22.9x (chain4, edge rows, embedding:
                                 err / bound 17.3, err / M 3.5e-5, RMS 1.1e-5 = 22.9x RMS_BOUND); every structural mutation
                                 (a tap dropped at one position, the halo one off, the mask carry, a shift swapped, the
                                 pool beyond L0, a tap mean over the wrong count, the previous row's shortcut) 1 200x and more
    RMS_BOUND = 2^-21 (4.8e-7)   largest emulated RMS 6.1e-8 -> 7.8x above it

    table-net kernels (5 variants x rows of 400 / 131 / 37 bases x both forms)
    TAB_GAMMA     = 6e-6         largest emulated err / M 1.3e-6 (average pool over 394 positions, matrix-core order of the
                                 f32 sum) -> 4.7x above it; the mutations reach err / M 0.03 - 2.6e7 (4 000x and more)
    TAB_RMS_BOUND = 2^-20        largest emulated RMS 1.8e-7 -> 5.3x above it; smallest mutation RMS 2.4e-3

The NMD ``eps`` of 1e-5 beside a mask count of dozens moves a tap mean by 1e-5 / 12 = 8e-7 relative at the least count a probe
window has - at the emulation's own error, so "eps left out" is not among the mutations; the coarser fault of the same kind, the
mean divided by ANOTHER layer's count (the "any" rule widens the mask by a position a side per layer), is.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import op_cases as oc

GAMMA = 2.0 ** -19
RMS_BOUND = 2.0 ** -21
TAB_GAMMA = 6e-6
TAB_RMS_BOUND = 2.0 ** -20

POS = 160            # positions of the small kernel's row image (five blocks of 32)
SPAN = 12            # codons a probe window holds

_BN = {"name": "masked_batchnorm", "config": {}}
_GELU = {"name": "activation", "config": {"activation": "gelu"}}
_NMD = {"name": "nmd"}


def _conv(k=3, padding="same"):
    return {"name": "masked_conv1d", "config": {"filters": 32, "kernel_size": k, "padding": padding, "use_bias": True}}


def _res(blocks=1):
    return {"name": "residual_block", "config": {"use_1x1conv": False, "block_size": blocks, "filters": 32, "kernel_size": 3,
                                                 "use_bias": True}}


# ---- the small-window family ------------------------------------------------------------------------------------------
#: variant -> what it is there for.  Codes are those of the switch in small_net_kernel (jg_small.hip): 8 last | 4 second
#: affine | 2 add | 1 save; "t" = the layer carries an NMD tap (the TAPS = true instantiation), L0 = the table layer.
SMALL_VARIANTS = {
    "baseline500":       "BASELINE configs[3]: TAPS = false; L0 save, codes 0, 3, 0, last + add + second affine (average pool)",
    "baseline500_max":   "the same with the max pool: last + add + second affine, PMAX",
    "baseline500_b1":    "one residual block: three layers, the weight fragments wrap round after two k = 3 convs",
    "baseline500_k3":    "first conv k0 = 3, SAME padding: pad0 = 1, L0 = L (160 positions at 160 codons)",
    "baseline500_k5":    "first conv k0 = 5, SAME padding: pad0 = 2",
    "baseline500_k3v":   "first conv k0 = 3, VALID padding: L0 = L - 2",
    "baseline500_nomask": "use_masking: false: no ballot masks, every position of [0, L0) pooled, id 0 a codon like any other",
    "nmdmerge500":       "the shipped two-tap model: TAPS = true, taps on L0 (save) and on the last layer (add + second affine)",
    "nmdmerge500_max":   "the same with the max pool: last + add + second affine, PMAX, beside an average tap of the same layer",
    "chain1":            "conv0, BN, GELU, nmd, [conv, BN, GELU, nmd] x 1: a tap on every layer; last without add / second affine",
    "chain2":            "... x 2: code 0 with a tap",
    "chain3":            "... x 3",
    "chain4":            "... x 4: five taps, the most the kernel holds",
    "chain2_max":        "chain2 with the max pool: last plain, PMAX, beside average taps",
    "chain3_plain":      "chain3 without nmd layers and reliability head: TAPS = false, code 0 and the plain last layer",
    "mix_a":             "conv0 t | res(1) | BN GELU nmd | conv BN GELU BN GELU nmd | conv BN GELU nmd: codes 0, 6 t, 4 t, last plain t",
    "mix_b":             "conv0 t | conv BN GELU BN GELU nmd | res(1) | nmd: codes 5 t, 0, last + add t",
    "mix_c":             "conv0 t | res(1) | BN GELU nmd | res(1) | nmd: codes 0, 7 t, 0, last + add t",
    "mix_d":             "conv0 t | res(1) | nmd | conv BN GELU BN GELU nmd: codes 0, 2 t, last + second affine t",
    "mix_e":             "conv0 | res(1) | nmd | res(1) | BN GELU nmd: L0 save without tap, codes 0, 3 t, 0, last + add + second affine t",
    "mix_f":             "conv0 t | conv BN GELU nmd | res(1) | BN GELU nmd: codes 1 t, 0, last + add + second affine t",
    "mix_b_max":         "mix_b with the max pool: last + add, PMAX, taps",
    "mix_d_max":         "mix_d with the max pool: last + second affine, PMAX, taps",
    "mix_c_plain":       "mix_c without taps: TAPS = false codes 7 and last + add",
    "mix_d_plain":       "mix_d without taps: TAPS = false codes 2 and last + second affine",
    "mix_a_plain":       "mix_a without taps: TAPS = false codes 6, 4 and the plain last layer",
    "mix_b_plain":       "mix_b without taps: TAPS = false code 5 and last + add",
    "mix_f_plain":       "mix_f without taps: TAPS = false code 1 and last + add + second affine",
    "chain2_plainmax":   "chain2 without taps, max pool: TAPS = false plain last layer, PMAX",
    "mix_b_plainmax":    "mix_b without taps, max pool: TAPS = false last + add, PMAX",
    "mix_d_plainmax":    "mix_d without taps, max pool: TAPS = false last + second affine, PMAX",
}


def small_cfg(name: str) -> dict:
    from conftest import load_model_cfg
    base, _, variant = name.partition("_")
    if base in ("baseline500", "nmdmerge500"):
        cfg = copy.deepcopy(load_model_cfg(base))
        rep = cfg["representation_learner"]
        c0 = rep["hidden_layers"][0]["config"]
        if variant == "max":
            rep["pooling"] = "max"
        elif variant == "b1":
            rep["hidden_layers"][3]["config"]["block_size"] = 1
        elif variant in ("k3", "k5"):
            c0["kernel_size"], c0["padding"] = int(variant[1]), "same"
        elif variant == "k3v":
            c0["kernel_size"] = 3
        elif variant in ("nomask", "nomaskmax"):           # (nomaskmax: the vector-tail test's unmasked max pool)
            cfg["use_masking"] = False
            if variant == "nomaskmax":
                rep["pooling"] = "max"
        elif variant:
            raise ValueError(name)
        return cfg
    cfg = copy.deepcopy(load_model_cfg("nmdmerge500"))
    cfg["reliability_model"].pop("input_shape", None)
    head = [_conv(7, "valid"), _BN, _GELU]
    if base.startswith("chain"):
        layers = head + [_NMD]
        for _ in range(int(base[5:])):
            layers += [_conv(), _BN, _GELU, _NMD]
    else:
        layers = {
            "a": head + [_NMD, _res(), _BN, _GELU, _NMD, _conv(), _BN, _GELU, _BN, _GELU, _NMD, _conv(), _BN, _GELU, _NMD],
            "b": head + [_NMD, _conv(), _BN, _GELU, _BN, _GELU, _NMD, _res(), _NMD],
            "c": head + [_NMD, _res(), _BN, _GELU, _NMD, _res(), _NMD],
            "d": head + [_NMD, _res(), _NMD, _conv(), _BN, _GELU, _BN, _GELU, _NMD],
            "e": head + [_res(), _NMD, _res(), _BN, _GELU, _NMD],
            "f": head + [_NMD, _conv(), _BN, _GELU, _NMD, _res(), _BN, _GELU, _NMD],
        }[variant[0]]
        variant = variant[2:]
    layers = copy.deepcopy(layers)
    if variant not in ("", "plain", "max", "plainmax"):
        raise ValueError(name)
    if variant.startswith("plain"):
        layers = [ly for ly in layers if ly["name"] != "nmd"]
        cfg.pop("reliability_model")
        cfg["reliability_out_dim"] = 0
    if variant.endswith("max"):
        cfg["representation_learner"]["pooling"] = "max"
    cfg["representation_learner"]["hidden_layers"] = layers
    return cfg


def compile_small(name: str, seed: int = 38341):
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    from oracle import forward as ofwd
    cfg = small_cfg(name)
    w = ofwd.random_weights(cfg, seed=seed)
    return cfg, w, compile_plan(build_plan(cfg), w)


class SmallNet:
    """The fused kernel's view of a program, restated from the op stages (jg_prepare.hip jg_prepare_small): per layer the first
    affine folded in f64 (scale, shift), add / save / second affine / tap, the pool kind; ``codes()`` = the switch codes."""

    def __init__(self, prog):
        from oracle import ops
        self.prog = prog
        self.pool_op = next(i for i, op in enumerate(prog.ops) if op.kind == ops.OP_POOL)
        self.convs = [i for i in range(self.pool_op) if prog.ops[i].kind == ops.OP_CONV]
        assert all(prog.ops[i].kind in (ops.OP_CONV, ops.OP_MASK, ops.OP_NMD_FINAL) for i in range(self.pool_op))
        c0 = prog.ops[self.convs[0]]
        assert c0.in_buf == ops.BUF_IDS and c0.cout == 32
        self.use_mask = c0.in_mask == ops.BUF_IDS
        self.k0, self.pad_same0 = c0.k, c0.padding == ops.PAD_SAME
        self.pool_kind = prog.ops[self.pool_op].arg
        self.layers = []
        blob = np.asarray(prog.blob, np.float64)
        for q, i in enumerate(self.convs):
            op = prog.ops[i]
            ly = dict(add=False, save=False, aff2=False, tap=None, s1=np.ones(32), t1=np.zeros(32), s2=np.ones(32), t2=np.zeros(32))
            st = 0

            def fold(sc, sh):
                nonlocal st
                while st < op.n_stages:
                    g = op.stages[st]
                    if g.kind == ops.ST_BIAS:
                        sh += blob[g.p0:g.p0 + 32]
                    elif g.kind == ops.ST_BN:
                        mu, inv, ga, be = (blob[p:p + 32] for p in (g.p0, g.p1, g.p2, g.p3))
                        sc *= inv * ga
                        sh[:] = (sh - mu) * inv * ga + be
                    else:
                        break
                    st += 1
            fold(ly["s1"], ly["t1"])
            if st < op.n_stages and op.stages[st].kind == ops.ST_ADD:
                src = max(r for r in range(q) if prog.ops[self.convs[r]].out_buf == op.stages[st].arg)
                self.layers[src]["save"] = True
                ly["add"] = True
                st += 1
            assert op.stages[st].kind == ops.ST_ACT and op.stages[st].arg == ops.ACT_GELU_TANH, (q, st)
            st += 1
            if st < op.n_stages and op.stages[st].kind in (ops.ST_BIAS, ops.ST_BN):
                fold(ly["s2"], ly["t2"])
                assert op.stages[st].kind == ops.ST_ACT and op.stages[st].arg == ops.ACT_GELU_TANH, (q, st)
                st += 1
                ly["aff2"] = True
            if st < op.n_stages and op.stages[st].kind == ops.ST_NMD:
                ly["tap"] = op.stages[st].arg
                st += 1
            assert st == op.n_stages, (q, st, op.n_stages)
            self.layers.append(ly)
        # every NMD finish in front of the pool: (op index, layer whose tap it finishes)
        self.finals = []
        for i in range(self.pool_op):
            op = prog.ops[i]
            if op.kind == ops.OP_NMD_FINAL:
                q = max(q for q, c in enumerate(self.convs) if c < i and self.layers[q]["tap"] == op.arg)
                self.finals.append((i, q))

    @property
    def n_conv(self) -> int:
        return len(self.convs) - 1

    def codes(self) -> list:
        """Per k = 3 layer the switch code of small_net_kernel, with "t" behind a tapped one; L0 as "L0[s][t]"."""
        out = ["L0" + ("s" if self.layers[0]["save"] else "") + ("t" if self.layers[0]["tap"] is not None else "")]
        for j, ly in enumerate(self.layers[1:]):
            last = j == self.n_conv - 1
            code = (8 if last else 0) | (4 if ly["aff2"] else 0) | (2 if ly["add"] else 0) | (0 if last else int(ly["save"]))
            out.append(str(code) + ("t" if ly["tap"] is not None else "") + ("m" if last and self.pool_kind == 0 else ""))
        return out

    def geometry(self, l: int):
        from oracle import ops
        return ops.conv_geometry(l, self.k0, 1, 1, ops.PAD_SAME if self.pad_same0 else ops.PAD_VALID)

    def full_length(self) -> int:
        """Codons per row that fill the kernel's 160 positions."""
        return POS if self.pad_same0 else POS + self.k0 - 1


def l0_aff2_cfg() -> dict:
    """conv0, BN, GELU, BN, GELU, conv, BN, GELU: a second affine behind the FIRST layer, which the fused kernel's table
    epilogue does not implement - the model must stay off the fused kernel."""
    cfg = small_cfg("chain1_plain")
    head = [_conv(7, "valid"), _BN, _GELU, _BN, _GELU, _conv(), _BN, _GELU]
    cfg["representation_learner"]["hidden_layers"] = copy.deepcopy(head)
    return cfg


# ---- inputs ---------------------------------------------------------------------------------------------------------
def probe_ids(l: int, starts=None, span: int = SPAN, vocab: int = 65, seed: int = 11) -> np.ndarray:
    """One window per start ``a``: ids valid in codons [a, a + span) of every frame, zero elsewhere."""
    rng = np.random.Generator(np.random.PCG64(seed))
    starts = list(range(l)) if starts is None else list(starts)
    ids = np.zeros((len(starts), 6, l), np.uint8)
    for w, a in enumerate(starts):
        b = min(a + span, l)
        ids[w, :, a:b] = rng.integers(1, vocab, (6, b - a))
    return ids


def ragged_ids(l: int, n_win: int = 24, vocab: int = 65, seed: int = 13) -> np.ndarray:
    """Windows that end early (zero tail) at every kind of length - for models without masks the tail is id 0's embedding."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(1, vocab, (n_win, 6, l)).astype(np.uint8)
    for w in range(n_win):
        ids[w, :, int(rng.integers(1, l + 1)):] = 0
    return ids


#: row classes of a multi-row set
ROW_CLASSES = ("full", "short<64", "mid", "long>128", "all-N", "probe", "N-runs")


def class_ids(cls: str, l: int, rng, vocab: int = 65) -> np.ndarray:
    """(6, l) ids of one window of a row class."""
    ids = rng.integers(1, vocab, (6, l)).astype(np.uint8)
    if cls == "short<64":
        ids[:, int(rng.integers(1, min(64, l))):] = 0
    elif cls == "mid":
        ids[:, int(rng.integers(min(64, l - 1), min(128, l))):] = 0
    elif cls == "long>128":
        ids[:, int(rng.integers(min(129, l - 1), l)):] = 0
    elif cls == "all-N":
        ids[:] = 0
    elif cls == "probe":
        a = int(rng.integers(0, l))
        keep = ids[:, a:a + SPAN].copy()
        ids[:] = 0
        ids[:, a:a + SPAN] = keep
    elif cls == "N-runs":
        for f in range(6):
            for a in rng.integers(0, l, 4):
                ids[f, a:a + int(rng.integers(1, 9))] = 0
    elif cls != "full":
        raise ValueError(cls)
    return ids


#: classes of the windows that the same wave meets on its first, second and third trip (then again from the first)
_TRIP_PATTERNS = (("full", "short<64", "full"), ("N-runs", "all-N", "long>128"), ("full", "probe", "mid"),
                  ("short<64", "long>128", "short<64"), ("long>128", "short<64", "probe"), ("mid", "full", "all-N"),
                  ("probe", "N-runs", "full"))


def multirow_ids(l: int, n_cu: int, rows_per_wg: int = 4, rows_per_win: int = 6, trips: float = 3.4, seed: int = 17, vocab: int = 65):
    """Enough windows for ONE launch group to take every wave (workgroup) of a persistent kernel with ``n_cu x rows_per_wg``
    rows in flight round its row loop ``trips`` times (3.4: three full trips and an uneven tail).  The window a wave meets on
    trip t lies a whole trip's windows behind the one it met on trip t - 1; their classes follow _TRIP_PATTERNS, so the rows a
    wave meets in sequence differ in the ways that expose stale state (full - short - full, an all-N row between two normal
    ones, a probe window behind a full one, the three ballot words in turn).  Returns (ids, class index per window)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    stride = n_cu * rows_per_wg
    n_win = int(np.ceil(trips * stride / rows_per_win)) + 1
    cls = np.zeros(n_win, np.int64)
    for w in range(n_win):
        t = w * rows_per_win // stride
        u = w - -(-t * stride // rows_per_win)
        cls[w] = ROW_CLASSES.index(_TRIP_PATTERNS[u % len(_TRIP_PATTERNS)][t % 3])
    ids = np.stack([class_ids(ROW_CLASSES[c], l, rng, vocab) for c in cls])
    return ids, cls


def probe_starts(l: int, dense: bool = True) -> list:
    """Every codon of the row; or (the CPU tier, where the arithmetic and not the position is measured) every third one plus
    the spans that cross position 0, the 32-position block edges, bits 63 / 64 and 127 / 128 of the mask words and the row end."""
    if dense:
        return list(range(l))
    special = [a for edge in (32, 64, 96, 128, 160) for a in range(edge - SPAN - 1, edge + 2)]
    return sorted({a for a in list(range(0, l, 3)) + special + list(range(l - SPAN - 2, l)) if 0 <= a < l})


def small_input_sets(net: "SmallNet", n_cu: int | None = None, dense_probes: bool = True) -> dict:
    """name -> (W, 6, l) ids of one variant: edge rows and probe windows at the full row length and at shorter ones, ragged
    windows, and - with ``n_cu`` - the multi-row set of a device with that many compute units."""
    l = net.full_length()
    sets = {f"edge rows l={l}": oc.edge_ids(l, n_win=12), "edge rows l=100": oc.edge_ids(100, n_win=12),
            "edge rows l=40": oc.edge_ids(40, n_win=12),
            f"probe windows l={l}": probe_ids(l, probe_starts(l, dense_probes)),
            "probe windows l=70": probe_ids(70, probe_starts(70, dense_probes), seed=12),
            f"ragged windows l={l}": ragged_ids(l)}
    if n_cu is not None:
        sets[f"multi-row set l={l}"] = multirow_ids(l, n_cu)[0]
    return sets


def trip_sample(n_win: int, rows_per_win: int, stride: int, cls=None, per_trip_rows: int = 256, seed: int = 29) -> np.ndarray:
    """Windows whose rows the float64 reference is evaluated on when a multi-row set is too large to compare whole: at least
    ``per_trip_rows`` rows from each of the first, second and third trip of the row loop (trip t = rows [t stride, (t + 1) stride)),
    every row class (``cls``: class per window) in each of them, the first window and the tail behind the last full trip; every
    window where a trip holds fewer rows than that (a device with few compute units)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_rows = n_win * rows_per_win
    trips = -(-n_rows // stride)
    need = -(-per_trip_rows // rows_per_win)
    pick = {0, n_win - 1}
    for t in range(trips):
        inside = [w for w in range(n_win) if w * rows_per_win >= t * stride and (w + 1) * rows_per_win <= min((t + 1) * stride, n_rows)]
        if t < 3:
            if len(inside) < need:           # a device with few compute units: a trip is smaller than the sample - compare every row
                return np.arange(n_win)
            pick |= set(rng.choice(inside, need, replace=False).tolist())
            if cls is not None:
                for c in set(cls.tolist()):
                    mine = [w for w in inside if cls[w] == c]
                    if mine:
                        pick.add(mine[int(rng.integers(len(mine)))])
        else:
            pick |= set(inside[-min(len(inside), 8):])
    return np.array(sorted(pick))


def wave_sequences(n_rows: int, stride: int) -> list:
    """Rows each wave (workgroup) meets, in order: wave r runs rows r, r + stride, r + 2 stride, ..."""
    return [list(range(r, n_rows, stride)) for r in range(min(stride, n_rows))]


def sequence_coverage(cls_per_row: np.ndarray, stride: int) -> dict:
    """What the row sequences of a multi-row set hold: trips per wave, and the transitions that expose stale state."""
    seqs = wave_sequences(len(cls_per_row), stride)
    name = [ROW_CLASSES[c] for c in cls_per_row]
    got = dict(min_trips=min(len(s) for s in seqs), max_trips=max(len(s) for s in seqs), full_short_full=0, n_between=0,
               probe_behind_full=0, words_in_turn=0)
    for s in seqs:
        for a, b, c in zip(s, s[1:], s[2:]):
            got["full_short_full"] += name[a] == "full" and name[b] == "short<64" and name[c] == "full"
            got["n_between"] += name[b] == "all-N" and name[a] not in ("all-N",) and name[c] not in ("all-N",)
        for a, b in zip(s, s[1:]):
            got["probe_behind_full"] += name[a] == "full" and name[b] == "probe"
            got["words_in_turn"] += {name[a], name[b]} == {"short<64", "long>128"}
    return got


# ---- the reference and the check ----------------------------------------------------------------------------------------
def _threads() -> int:
    from conftest import _cpu_quota
    return max(1, min(_cpu_quota(), 16))


def by_windows(fn, ids: np.ndarray, per: int = 32) -> dict:
    """``fn(ids) -> {name: array or tuple of arrays, one row per window}`` over blocks of ``per`` windows on a thread pool
    (windows are independent; numpy releases the interpreter lock, and blocks this small stay in the caches)."""
    from concurrent.futures import ThreadPoolExecutor
    blocks = [ids[i:i + per] for i in range(0, len(ids), per)]
    with ThreadPoolExecutor(_threads()) as pool:
        outs = list(pool.map(fn, blocks))
    cat = lambda parts: np.concatenate(parts, axis=0)   # noqa: E731
    return {k: tuple(cat([o[k][j] for o in outs]) for j in range(len(v))) if isinstance(v, tuple) else cat([o[k] for o in outs])
            for k, v in outs[0].items()}


def reference(prog, ids: np.ndarray) -> dict:
    """{"embedding": (ref, M), "nmd": (ref, M)} per window, from oracle/ops.py chained from the ids: the pool op's and every
    NMD finish's float64 result and magnitude, laid out like the model's output vectors (a two-strand model: per strand row)."""
    return by_windows(lambda block: _reference(prog, block), ids)


def _reference(prog, ids: np.ndarray) -> dict:
    from oracle import ops
    keep = [i for i, op in enumerate(prog.ops) if op.kind in (ops.OP_POOL, ops.OP_NMD_FINAL)]
    state = ops.State(ops.program_rows(prog, ids))
    res, mags = {}, {}
    for i, op in enumerate(prog.ops):
        if op.kind == ops.OP_STRANDS:
            continue
        # the pool reads its producer's magnitude (the convs keep reading |x|: each is bounded in its own input's scale)
        state.M = {op.in_buf: mags[op.in_buf]} if op.kind == ops.OP_POOL and op.in_buf in mags else {}
        r = ops.run_op(prog, i, state)
        ops.apply(prog, i, state, r)
        if op.kind in (ops.OP_CONV, ops.OP_ELTWISE):
            mags[op.out_buf] = r.M
        if i in keep:
            res[i] = r
    out = {}
    for slot, name in ((ops.VEC_EMBEDDING, "embedding"), (ops.VEC_NMD, "nmd")):
        mine = [i for i in keep if prog.ops[i].out_vec == slot]
        if not mine:
            continue
        width = max(prog.ops[i].vec_off + res[i].out.shape[1] for i in mine)
        ref = np.zeros((res[mine[0]].out.shape[0], width))
        mag = np.zeros_like(ref)
        for i in mine:
            o = prog.ops[i].vec_off
            ref[:, o:o + res[i].out.shape[1]] = res[i].out
            mag[:, o:o + res[i].out.shape[1]] = res[i].M
        out[name] = (ref, mag)
    return out


def check_vec(got, ref, M, gamma=None, rms_bound=None):
    """op_cases.check on (rows, width) vectors with this module's constants -> (CheckResult, ok)."""
    gamma = GAMMA if gamma is None else gamma
    rms_bound = RMS_BOUND if rms_bound is None else rms_bound
    res = oc.check(np.asarray(got)[:, None, None, :], ref[:, None, None, :], M[:, None, None, :], gamma=gamma)
    return res, (res.n_bad == 0 and res.rms <= rms_bound)


def report(what: str, res, gamma=None, rms_bound=None) -> str:
    gamma = GAMMA if gamma is None else gamma
    rms_bound = RMS_BOUND if rms_bound is None else rms_bound
    return (f"{what}: worst err/bound {res.worst:.3g}, worst err/M {res.worst_m:.3g} (GAMMA {gamma:.3g}), rms err/M {res.rms:.3g} "
            f"(bound {rms_bound:.3g}), {res.n_bad} elements out; worst (window, -, -, -, channel, err/M): {res.offenders[:3]}")


# ---- numpy emulation of small_net_kernel ----------------------------------------------------------------------------------
_F = np.float32


def _gelu32(x):
    """gelu_stages of jg_small.hip in f32: x / (1 + 2^(x (c0 + c1 x^2)))."""
    t = (x * x).astype(_F)
    t = (_F(-2.3022082) + _F(-0.10294324) * t).astype(_F)
    t = (x * t).astype(_F)
    with np.errstate(over="ignore"):
        t = np.exp2(t).astype(_F)
    t = (t + _F(1.0)).astype(_F)
    t = (_F(1.0) / t).astype(_F)
    return (x * t).astype(_F)


def _lane_reduce(v, maximum=False):
    """row_reduce_store: (R, 160, 32) per-position values (already masked) -> (R, 32): a lane adds its five blocks in turn, the
    32 lanes combine in a butterfly (xor 16, 8, 4, 2, 1)."""
    r = v.shape[0]
    v = v.reshape(r, 5, 32, 32)
    acc = v[:, 0]
    for b in range(1, 5):
        acc = np.maximum(acc, v[:, b]) if maximum else (acc + v[:, b]).astype(_F)
    n = 32
    while n > 1:
        n //= 2
        acc = np.maximum(acc[:, :n], acc[:, n:2 * n]) if maximum else (acc[:, :n] + acc[:, n:2 * n]).astype(_F)
    return acc[:, 0]


def emulate_small(net: SmallNet, ids: np.ndarray, mut: dict | None = None) -> dict:
    """``_emulate_small`` over blocks of windows on a thread pool."""
    return by_windows(lambda block: _emulate_small(net, block, mut), ids)


def _emulate_small(net: SmallNet, ids: np.ndarray, mut: dict | None = None) -> dict:
    """small_net_kernel + small_pool_final_kernel in numpy as the source states them: the f32 first-layer table (E . W_t in
    f64, times the folded scale, the shift on tap 0's rows) summed tap by tap; the k = 3 weights times the first affine's scale
    (f64), split hi / lo without a pre-scale; hi_w hi_x + hi_w lo_x + lo_w hi_x per tap and 16-channel chunk accumulated in f32
    on top of the shift; the epilogue in f32; the row image re-split to hi / lo (masked) between layers; f32 pool / tap sums
    and the final divide.  ``mut``: one mutation (see MUTATIONS).  Returns {"embedding": (W, 32), "nmd": (W, 32 x taps)}."""
    from oracle import ops
    mut = mut or {}
    prog = net.prog
    blob = np.asarray(prog.blob, np.float64)
    ids = np.asarray(ids)
    n_win, frames, l = ids.shape
    rows = ids.reshape(-1, l).astype(np.int64)
    r = rows.shape[0]
    l0, pad0 = net.geometry(l)
    assert 1 <= l0 <= POS and l <= 192
    vocab = prog.vocab
    c0 = prog.ops[net.convs[0]]
    # the table
    cin_pad = (c0.cin + 1) & ~1
    emb = blob[c0.b_off:c0.b_off + vocab * c0.cin].reshape(vocab, c0.cin)
    w0 = blob[c0.w_off:c0.w_off + c0.k * cin_pad * 32].reshape(c0.k, cin_pad, 32)[:, :c0.cin]
    lut = np.zeros((c0.k, vocab + 1, 32), _F)
    first = 1 if net.use_mask else 0
    lut[:, first:vocab] = (np.einsum("ic,tcn->tin", emb[first:], w0) * net.layers[0]["s1"]).astype(_F)
    if mut.get("kind") == "zero_id_contributes":
        lut[:, 0] = (np.einsum("c,tcn->tn", emb[0], w0) * net.layers[0]["s1"]).astype(_F)
    lut[0] = (lut[0].astype(np.float64) + net.layers[0]["t1"]).astype(_F)
    # ids with margins: index IDM + q, padding = row `vocab`
    idm = 8
    idbuf = np.full((r, 224), vocab, np.int64)
    idbuf[:, idm:idm + l] = rows
    acc = np.zeros((r, POS, 32), _F)
    p = np.arange(POS)
    for t in range(c0.k):
        acc = (acc + lut[t][idbuf[:, idm + p + t - pad0]]).astype(_F)
    # masks as (r, 192) booleans
    valid0 = np.arange(192) < l0
    m = np.zeros((r, 192), bool)
    m[:, :l] = (rows != 0) if net.use_mask else True
    if net.use_mask:
        mo = np.zeros_like(m)
        for t in range(c0.k):
            s = t - pad0                       # bit p of the result = bit p + s of m
            sh = np.zeros_like(m)
            if s >= 0:
                sh[:, :192 - s] = m[:, s:]
            else:
                sh[:, -s:] = m[:, :192 + s]
            mo |= sh
    else:
        mo = m.copy()
    mo &= valid0

    def split(x):                              # (torch: numpy's f32 -> f16 conversion is ten times slower)
        xt = torch.from_numpy(np.ascontiguousarray(x, _F))
        hi = xt.half()
        lo = (xt - hi.float()).half()
        return hi.numpy(), lo.numpy()

    def mm(a, b):                              # f32 product, f32 accumulation (torch: see oracle/ops.py shifted_sum)
        return (torch.from_numpy(a) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()

    parts = {}            # layer -> (sums (r, 32), count (r,))
    counts = {}

    def out_step(q, x, mo):
        keep = mo[:, :POS, None]
        ly = net.layers[q]
        counts[q] = mo.sum(axis=1).astype(_F)
        if ly["tap"] is not None:
            parts[q] = _lane_reduce(np.where(keep, x, _F(0)).astype(_F))
        hi, lo = split(x)
        return np.where(keep, hi, np.float16(0)), np.where(keep, lo, np.float16(0))

    x = _gelu32(acc)
    sc = x if net.layers[0]["save"] else None
    xh, xl = out_step(0, x, mo)
    pooled = None
    nc = net.n_conv
    for j in range(nc):
        q = j + 1
        ly = net.layers[q]
        op = prog.ops[net.convs[q]]
        if net.use_mask:
            shl = np.zeros_like(mo)
            shl[:, 1:] = mo[:, :-1]
            shr = np.zeros_like(mo)
            shr[:, :-1] = mo[:, 1:]
            if mut.get("kind") == "mask_carry" and mut["layer"] == q:
                shl[:, 64] = False
            mo = (shl | mo | shr) & valid0
            if mut.get("kind") == "pool_beyond_l0" and j == nc - 1:
                mo = (shl | mo | shr) & (np.arange(192) < POS)
        elif mut.get("kind") == "pool_beyond_l0" and j == nc - 1:
            mo = np.broadcast_to(np.arange(192) < min(l0 + 1, POS), mo.shape).copy()
        w = blob[op.w_off:op.w_off + 3 * 32 * 32].reshape(3, 32, 32)
        wf = (w * ly["s1"]).astype(_F)
        wh, wl = split(wf)
        wh, wl = wh.astype(_F), wl.astype(_F)
        # row image with halo rows -1 and 160
        ih = np.zeros((r, POS + 2, 32), _F)
        il = np.zeros((r, POS + 2, 32), _F)
        ih[:, 1:POS + 1], il[:, 1:POS + 1] = xh.astype(_F), xl.astype(_F)
        acc = np.broadcast_to(ly["t1"].astype(_F), (r, POS, 32)).copy()
        for t in range(3):
            t_h, t_l = ih[:, t:t + POS].copy(), il[:, t:t + POS].copy()      # image rows of positions p + t - 1
            if mut.get("kind") == "halo_off" and mut["layer"] == q and t == 0:
                t_h[:, mut["pos"]], t_l[:, mut["pos"]] = ih[:, mut["pos"] - 1], il[:, mut["pos"] - 1]
            t_h, t_l = t_h.reshape(-1, 32), t_l.reshape(-1, 32)
            for cc in range(2):
                ch = slice(cc * 16, cc * 16 + 16)
                a_h, a_l = np.ascontiguousarray(t_h[:, ch]), np.ascontiguousarray(t_l[:, ch])
                terms = [mm(a_h, wh[t, ch]), mm(a_l, wh[t, ch])]
                if not (mut.get("kind") == "drop_cross" and mut["layer"] == q):
                    terms.append(mm(a_h, wl[t, ch]))
                for term in terms:
                    term = term.reshape(r, POS, 32)
                    if mut.get("kind") == "drop_tap" and mut["layer"] == q and mut["tap"] == t:
                        term[:, mut["pos"]] = 0
                    acc = (acc + term).astype(_F)
        x = acc
        if ly["add"]:
            s_ = sc
            if mut.get("kind") == "sc_hi_only" and mut["layer"] == q:
                s_ = s_.astype(np.float16).astype(_F)
            if mut.get("kind") == "sc_prev_row" and mut["layer"] == q:
                s_ = np.roll(s_, 1, axis=0)
            x = (x + s_).astype(_F)
        x = _gelu32(x)
        if ly["aff2"]:
            t2 = ly["t2"].astype(_F)
            if mut.get("kind") == "t2_swap" and mut["layer"] == q:
                t2 = t2.copy()
                t2[[mut["a"], mut["b"]]] = t2[[mut["b"], mut["a"]]]
            x = _gelu32((x * ly["s2"].astype(_F) + t2).astype(_F))
        if ly["save"]:
            sc = x
        if j < nc - 1:
            xh, xl = out_step(q, x, mo)
        else:
            keep = mo[:, :POS, None]
            counts[q] = mo.sum(axis=1).astype(_F)
            if ly["tap"] is not None:
                parts[q] = _lane_reduce(np.where(keep, x, _F(0)).astype(_F))
            if net.pool_kind == ops.POOL_AVG:
                pooled = _lane_reduce(np.where(keep, x, _F(0)).astype(_F))
            else:
                pooled = np.maximum(_lane_reduce(np.where(keep, x, _F(-1.0e9)).astype(_F), maximum=True), _F(-1.0e9))
    # small_pool_final_kernel: the six frames of a window in turn
    last = nc

    def frames_sum(v):
        v = v.reshape(n_win, frames, *v.shape[1:])
        acc = v[:, 0]
        for f in range(1, frames):
            acc = (acc + v[:, f]).astype(_F)
        return acc

    cnt = frames_sum(counts[last])
    if net.pool_kind == ops.POOL_AVG:
        emb_out = (frames_sum(pooled) / np.maximum(cnt, _F(1e-7))[:, None]).astype(_F)
    else:
        emb_out = np.where(cnt[:, None] > 0, pooled.reshape(n_win, frames, 32).max(axis=1), _F(0)).astype(_F)
    out = {"embedding": emb_out}
    if net.finals:
        width = max(prog.ops[i].vec_off + 32 for i, _ in net.finals)
        nmd = np.zeros((n_win, width), _F)
        for i, q in net.finals:
            op = prog.ops[i]
            cq = counts[last] if mut.get("kind") == "tap_count_last" else counts[q]
            mm = blob[op.b_off:op.b_off + 32].astype(_F)
            v = (frames_sum(parts[q]) / (frames_sum(cq) + _F(op.f0))[:, None]).astype(_F)
            nmd[:, op.vec_off:op.vec_off + 32] = (v - mm).astype(_F)
        out["nmd"] = nmd
    return out


def small_mutations(net: SmallNet, l0: int) -> dict:
    """name -> mutation of ``emulate_small`` for a net with three or more k = 3 layers (first / middle / last)."""
    nc = net.n_conv
    layers = {"first": 1, "middle": (nc + 1) // 2 if nc > 2 else None, "last": nc}
    muts = {}
    for where, q in layers.items():
        if q is None:
            continue
        for pos in (0, 31, 32, 63, 64, 127, 128, l0 - 1):
            muts[f"tap 1 dropped at position {pos} of the {where} k=3 layer"] = dict(kind="drop_tap", layer=q, tap=1, pos=pos)
    muts["halo read one position off across the block edge (position 32, tap 0)"] = dict(kind="halo_off", layer=1, pos=32)
    muts["halo read one position off across the block edge (position 128, tap 0, last layer)"] = dict(kind="halo_off", layer=nc, pos=128)
    if net.use_mask:
        muts["'any' mask rule loses the carry across bit 64"] = dict(kind="mask_carry", layer=1)
        muts["tap mean divided by the last layer's mask count"] = dict(kind="tap_count_last")
    add = [q for q in range(1, nc + 1) if net.layers[q]["add"]]
    if add:
        muts["shortcut's lo half dropped"] = dict(kind="sc_hi_only", layer=add[0])
        muts["shortcut taken from the previous row"] = dict(kind="sc_prev_row", layer=add[-1])
    muts["hi_x lo_w dropped in one layer"] = dict(kind="drop_cross", layer=max(1, nc // 2))
    aff2 = [q for q in range(1, nc + 1) if net.layers[q]["aff2"]]
    if aff2:
        muts["second affine's shift swapped between channels 5 and 6"] = dict(kind="t2_swap", layer=aff2[0], a=5, b=6)
    muts["pool counts positions at or beyond L0"] = dict(kind="pool_beyond_l0")
    return muts


# ---- the table-net strand kernels -------------------------------------------------------------------------------------------
#: variant -> (branch layers, pooling, what it is there for)
TAB_VARIANTS = {
    "dvf500":      "the shipped model: k = 10, 500 filters, ReLU, max pool: bias + activation behind the pool (LATE), KS = 3",
    "avg_gelu":    "k = 7, 64 filters, GELU, average pool: activation per position, the sum and the divide by L_out, KS = 2",
    "same_dil":    "k = 6, SAME padding, dilation 3, 100 filters, sigmoid, max pool: pad_left, taps outside the strand",
    "max_gelu":    "k = 4, GELU (not monotone) + max pool: activation per position in front of the max, KS = 1",
    "tanh_k13":    "k = 13, tanh, max pool: KS = 4",
}


def tab_cfg(name: str) -> dict:
    from conftest import load_model_cfg
    cfg = copy.deepcopy(load_model_cfg("dvf500"))
    if name == "dvf500":
        return cfg
    branch = {
        "avg_gelu": ([{"name": "conv1d", "config": {"filters": 64, "kernel_size": 7, "activation": "gelu"}}], "average1d"),
        "same_dil": ([{"name": "conv1d", "config": {"filters": 100, "kernel_size": 6, "padding": "same", "dilation_rate": 3}},
                      {"name": "sigmoid"}], "max1d"),
        "max_gelu": ([{"name": "conv1d", "config": {"filters": 96, "kernel_size": 4, "activation": "gelu"}}], "max1d"),
        "tanh_k13": ([{"name": "conv1d", "config": {"filters": 128, "kernel_size": 13}}, {"name": "tanh"}], "max1d"),
    }[name]
    cfg["representation_learner"]["branch"] = {"hidden_layers": branch[0], "pooling": branch[1]}
    cfg["classifier"]["branch"]["hidden_layers"] = [
        {"name": "dense", "config": {"units": 3}}, {"name": "merge", "config": {"method": "average"}}]
    return cfg


def compile_tab(name: str, seed: int = 38341):
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    from oracle import strands as ost
    cfg = tab_cfg(name)
    w = ost.random_weights(cfg, seed=seed)
    return cfg, w, compile_plan(build_plan(cfg), w)


def strand_ids(n_win: int, l: int, seed: int = 19, n_frac: float = 0.03) -> np.ndarray:
    """(n_win, 2, l) nucleotide ids 1 .. 4 (0 = N or padding): N runs, ragged tails, an all-N window, N at both row ends."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(1, 5, (n_win, 2, l)).astype(np.uint8)
    ids[rng.random(ids.shape) < n_frac] = 0
    for w in range(n_win):
        if w % 5 == 1:
            ids[w, :, int(rng.integers(l // 4, l)):] = 0
        if w % 5 == 2:
            ids[w, :, :int(rng.integers(1, 20))] = 0
        if w % 7 == 3:
            ids[w, :, -int(rng.integers(1, 20)):] = 0
    if n_win > 4:
        ids[4] = 0
    return ids


def strand_multirow_ids(l: int, n_cu: int, wg_per_cu: int = 2, trips: float = 3.25, seed: int = 23) -> np.ndarray:
    """Strand windows for one launch group that takes every workgroup of the strand kernels (at most ``wg_per_cu`` per CU, one
    row each) round its row loop three times, a part of them a fourth time: both parities of the double-buffered id image, and
    last rows without a successor behind an odd and behind an even number of trips.  Neighbouring rows differ (strand_ids)."""
    n_rows = int(trips * wg_per_cu * n_cu) | 1
    return strand_ids((n_rows + 1) // 2 + 1, l, seed=seed)


def emulate_tab(prog, ids: np.ndarray, lds: bool, mut: str | None = None) -> np.ndarray:
    """The strand branch's conv + bias + activation + pool per strand row as the two kernels compute it.  Matrix-core form
    (jg_tabnet.hip): one-hot ids (exact in f16) times the weights split hi / lo f16 without a pre-scale, both products
    accumulated in f32 tap by tap, bias and activation per position - or behind the max where the activation is monotone -,
    f32 pool.  LDS-table form (tab_conv_pool_kernel): f32 table rows added tap by tap on top of the bias.  -> (rows, cout)."""
    from oracle import ops
    conv = next(op for op in prog.ops if op.kind == ops.OP_CONV)
    pool = next(op for op in prog.ops if op.kind == ops.OP_POOL)
    blob = np.asarray(prog.blob, np.float64)
    rows = ops.program_rows(prog, ids)[:, 0].astype(np.int64)
    r, l = rows.shape
    table = blob[conv.b_off:conv.b_off + prog.vocab * conv.cin].reshape(prog.vocab, conv.cin)
    w = ops.conv_weights(prog, conv)
    lo, pl = ops.conv_geometry(l, conv.k, 1, conv.dilation, conv.padding)
    if mut == "same_as_valid_left":
        pl = 0
    tw = np.einsum("vc,tcn->tvn", table, w).astype(_F)           # per tap: the table row of each id
    if mut != "zero_id_contributes":
        tw[:, 0] = 0
    else:
        tw[:, 0] = tw[:, 1]
    if lds:
        parts = [(tw, None)]
    else:
        hi = tw.astype(np.float16)
        parts = [(hi.astype(_F), None), ((tw - hi.astype(_F)).astype(np.float16).astype(_F), None)]
    bias = np.zeros(conv.cout, _F)
    acts = []
    for s in range(conv.n_stages):
        st = conv.stages[s]
        if st.kind == ops.ST_BIAS:
            bias = blob[st.p0:st.p0 + conv.cout].astype(_F)
        elif st.kind == ops.ST_ACT:
            acts.append(st.arg)
    act = acts[0] if acts else ops.ACT_NONE
    acc = np.broadcast_to(bias if lds else _F(0), (r, lo, conv.cout)).astype(_F).copy()
    m = np.arange(lo)
    for t in range(conv.k):
        src = m + t * conv.dilation - pl
        if mut == "last_tap_one_early" and t == conv.k - 1:
            src = np.where(m == lo - 1, src - 1, src)
        ok = (src >= 0) & (src < l)
        idt = np.where(ok[None, :], rows[:, np.clip(src, 0, l - 1)], 0)
        for plane, _ in parts:
            acc = (acc + plane[t][idt]).astype(_F)

    def f_act(v):
        return ops.act(act, v.astype(np.float64)).astype(_F)       # (the activation itself in f64, rounded: its own error is
                                                                     # a few ulp in the kernels' approximations)
    late = (not lds) and pool.arg != ops.POOL_AVG and act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH, ops.ACT_SIGMOID)
    if late:
        return f_act((acc.max(axis=1) + bias).astype(_F))
    v = f_act(acc if lds else (acc + bias).astype(_F))
    if pool.arg == ops.POOL_AVG:
        # the order of the f32 sum.  Matrix cores: a lane adds the sixteen positions it holds of each 32-block in turn, block
        # after block, then the wave's two halves are added.  LDS form: 1024 / lanes groups of threads take blocks of four
        # consecutive positions in turn, then the groups' partial sums are added one after the other.
        if lds:
            cq = (conv.cout + 3) // 4
            groups = 1024 // (64 if cq <= 64 else 128 if cq <= 128 else 256)
            orders = [[p + j for p in range(g * 4, lo, groups * 4) for j in range(4) if p + j < lo] for g in range(groups)]
        else:
            nb = (lo + 31) // 32
            orders = [[q for b in range(nb) for i in range(16) for q in [32 * b + (i >> 2) * 8 + hh * 4 + (i & 3)] if q < lo]
                      for hh in range(2)]
        total = None
        for order in orders:
            part = np.zeros((r, conv.cout), _F)
            for q in order:
                part = (part + v[:, q]).astype(_F)
            total = part if total is None else (total + part).astype(_F)
        return (total / _F(lo)).astype(_F)
    return v.max(axis=1)


TAB_MUTATIONS = {"the last tap read one id early at the row end": "last_tap_one_early",
                 "SAME padding treated as VALID at the left edge": "same_as_valid_left",
                 "the zero id not contributing zero": "zero_id_contributes"}
