"""The case matrix of the fused residual-block kernels (tests/test_resblock_reference.py on the CPU,
tests/test_gpu_resblocks.py on the GPU): ``resblock32_kernel<K>`` (jg_resblock.hip) and ``resblock64_kernel<K, D>``
(jg_resblock64.hip) run conv1, the re-split intermediate in LDS, conv2, the shortcut and the GELU in one launch.

A case is the smallest program that puts ONE block on a fused kernel, written as an op list (``_Writer`` of
tests/conv_instance_cases.py): a first-layer conv from the ids makes the block input x with C channels and [bias, GELU] - no
mask multiply, so x is non-zero at masked positions, which tells "shortcut = x" from "shortcut = x m0"; a mask op; conv1
[bias, bn, GELU]; the mask op between the convs; conv2 [bias, bn, ADD x, GELU]; a reader that fixes the store form (``f16s``:
a stride-1 split-f16 conv; ``psplit``: a five-tap and a 1x1 stride-2 conv only); a pool and a dense layer.

Tiling, restated (the CPU module parses the sources and fails when they differ): nb = 4 blocks of 32 intermediate positions at
32 channels, 2 at 64; RH = 32 nb, halo = (k - 1) d, T = tile_out = RH - halo, pad = halo / 2; units = rows x ceil(L / T), the
grid min(units, 2 n_cu) at 32 channels and min(units, n_cu) at 64.  Tile borders therefore fall every T positions - not at
256, where op_cases.edge_ids places its mask changes: ``tile_edge_ids`` places them at T and 2 T instead.

Masks: m0 = conv1's input mask, m1 = the mask between the convs, m2 = conv2's output mask (multiplied in only by the
phase-split store).  ``any``: m1 grows past m0 - live outputs with m0 = 0 take the shortcut from HBM (the LDS image holds
conv1's masked zero there); ``strict``: m1 shrinks - positions with m0 = 1 and m1 = 0; ``none``: the convs carry no mask,
every mask pointer of the kernel is null (another count in the 64-channel kernel's counted wait).

With the default 12 windows (72 rows, at most 3 tiles each) every case has fewer units than the grid; the ``launch`` cases
size their window count from the device's compute-unit count (``launch_windows``).

What a shape cannot contain (``required_classes``): a row of one position has no tile border and nothing to shift; L <= T has
no second tile; an unmasked block has no masked position of any kind; m2 and the odd row end count only for a phase-split
store.  Every other class of the census must be present in every case.

Margins of the split-f16 emulation and of the weakest mutation per geometry (tests/test_resblock_reference.py prints this
table; err / bound of op_cases.check, <= 0.25 required of the emulation, >= 8 of every mutation; rms as a fraction of
RMS_BOUND):

  c32 k5 d1   9 cases  emulation err/bound  0.019  err/M 1.23e-07 (GAMMA / 48.9)  rms  0.022   weakest mutation  5.13e+03 (shortcut_m0)
  c32 k5 d2   8 cases  emulation err/bound  0.023  err/M 1.47e-07 (GAMMA / 40.8)  rms  0.045   weakest mutation   5.1e+03 (outside)
  c32 k5 d3   6 cases  emulation err/bound  0.021  err/M 1.37e-07 (GAMMA / 43.8)  rms  0.023   weakest mutation  1.91e+04 (shift)
  c32 k5 d8   6 cases  emulation err/bound  0.024  err/M 1.53e-07 (GAMMA / 39.2)  rms  0.044   weakest mutation  1.31e+04 (shift)
  c32 k3 d1   7 cases  emulation err/bound  0.021  err/M 1.34e-07 (GAMMA / 44.8)  rms  0.025   weakest mutation  4.61e+03 (outside)
  c32 k3 d2   9 cases  emulation err/bound  0.021  err/M 1.35e-07 (GAMMA / 44.6)  rms  0.048   weakest mutation  3.88e+03 (shortcut_m0)
  c32 k3 d7   6 cases  emulation err/bound  0.021  err/M 1.34e-07 (GAMMA / 44.8)  rms  0.021   weakest mutation  2.78e+04 (shortcut_m0)
  c32 k3 d16  6 cases  emulation err/bound  0.027  err/M 1.77e-07 (GAMMA / 34.0)  rms  0.048   weakest mutation  3.42e+04 (shortcut_m0)
  c64 k5 d1   8 cases  emulation err/bound  0.021  err/M 1.34e-07 (GAMMA / 44.9)  rms  0.020   weakest mutation  2.88e+03 (outside)
  c64 k5 d2  13 cases  emulation err/bound  0.025  err/M 1.63e-07 (GAMMA / 36.8)  rms  0.044   weakest mutation  2.62e+03 (outside)
  c64 k3 d1  10 cases  emulation err/bound  0.017  err/M 1.12e-07 (GAMMA / 53.8)  rms  0.017   weakest mutation  1.27e+03 (shortcut_m0)
  c64 k3 d2   8 cases  emulation err/bound  0.020  err/M 1.31e-07 (GAMMA / 45.6)  rms  0.053   weakest mutation  4.21e+03 (outside)
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

from conv_instance_cases import ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, EMB, VOCAB, _Writer

# ---- the tiling and the support predicates, restated ---------------------------------------------------------------------------
NB = {32: 4, 64: 2}                 # RB_NB, R6_NB
XR, OR = 5, 3                       # R6_XR, R6_OR: image slots and bit slots of the 64-channel pipeline


@dataclass(frozen=True)
class Tiling:
    nb: int
    RH: int
    halo: int
    T: int
    pad: int
    tiles: int


def tiling(c: int, k: int, d: int, l: int) -> Tiling:
    """jg_resblock_tiling / jg_resblock64_tiling."""
    nb = NB[c]
    halo = (k - 1) * d
    T = 32 * nb - halo
    return Tiling(nb, 32 * nb, halo, T, halo // 2, -(-l // T))


def supports32(c: int, k: int, d: int) -> bool:
    """jg_resblock_supports."""
    return c == 32 and k in (5, 3) and d >= 1 and (k - 1) * d <= 32


def smem64(k: int, d: int) -> int:
    """r6_smem."""
    rx = 64 + (k - 1) * d
    x_slot = (16 * rx + 63) & ~63
    return (XR * x_slot + 2 * 16 * 64) * 16 + 4 * 64 * 4 + (OR * 64 + OR) * 4


def supports64(c: int, k: int, d: int) -> bool:
    """jg_resblock64_supports."""
    return c == 64 and k in (5, 3) and d in (1, 2) and smem64(k, d) <= 160 * 1024


def supports(c: int, k: int, d: int) -> bool:
    return supports32(c, k, d) or supports64(c, k, d)


def grid(c: int, units: int, n_cu: int) -> int:
    """jg_launch_resblock / jg_launch_resblock64."""
    return min(units, 2 * n_cu if c == 32 else n_cu)


#: (channels, taps, dilation): d up to the predicate's limit on the 32-channel kernel, all four 64-channel instantiations
GEOMETRIES = [(32, 5, 1), (32, 5, 2), (32, 5, 3), (32, 5, 8), (32, 3, 1), (32, 3, 2), (32, 3, 7), (32, 3, 16),
              (64, 5, 1), (64, 5, 2), (64, 3, 1), (64, 3, 2)]
#: geometry -> (the placement rule describe() names, ...): a geometry the support predicate accepts but an earlier rule keeps
#: off the fused kernel is asserted unfused and right layer by layer, like an UNREACHABLE conv instance.  None is known.
PLACED_ELSEWHERE: dict = {}


# ---- cases ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    c: int
    k: int
    d: int
    l: int
    masks: str = "any"             # any / strict / none
    store: str = "f16s"            # f16s / psplit
    n_win: int = 12
    chunk: int = 0
    act: int = ACT_GELU_TANH
    neg: str | None = None         # the reason the placement must not fuse this program
    launch: float | None = None    # units / grid the window count is sized for on the device (launch_windows)
    gain1: float = 1.6             # kernel gains of conv1 / conv2 (the range-guard cases scale them)
    gain2: float = 1.6
    guard: bool = False

    @property
    def geometry(self):
        return (self.c, self.k, self.d)

    @property
    def til(self) -> Tiling:
        return tiling(self.c, self.k, self.d, self.l)

    @property
    def fused(self) -> bool:
        return self.neg is None and self.geometry not in PLACED_ELSEWHERE


def launch_windows(c: Case, n_cu: int) -> int:
    """Windows of a launch-shape case: about ``c.launch`` x grid units, never a multiple of the grid - neighbouring
    workgroups then take floor and ceil of it tiles."""
    per_win = 6 * c.til.tiles
    g = 2 * n_cu if c.c == 32 else n_cu
    n = -(-int(c.launch * g) // per_win) + 1
    while (n * per_win) % g == 0 or n * per_win <= g:
        n += 1
    return n


def n_local_range(c: Case, n_win: int, n_cu: int) -> tuple:
    """(fewest, most) tiles a workgroup of the launch takes."""
    units = 6 * n_win * c.til.tiles
    g = grid(c.c, units, n_cu)
    return units // g, -(-units // g)


def _cases() -> list:
    out = []

    def add(tag, c, k, d, l, **kw):
        name = f"c{c}-k{k}-d{d}-l{l}-{kw.get('masks', 'any')}" + ("-psplit" if kw.get("store") == "psplit" else "") + (f"-{tag}" if tag else "")
        out.append(Case(name, c, k, d, l, **kw))

    for gi, (c, k, d) in enumerate(GEOMETRIES):
        T = tiling(c, k, d, 1).T
        # one position / one full tile: the mask forms alternate; a second tile of one position / three tiles: both forms
        add("", c, k, d, 1, masks=("any", "strict")[gi % 2])
        add("", c, k, d, T, masks=("strict", "any")[gi % 2])
        for l in (T + 1, 2 * T + 1):
            for masks in ("any", "strict"):
                add("", c, k, d, l, masks=masks)
    # no masks at all: one geometry per 32-channel template, every 64-channel instantiation (n_vm of its counted wait)
    for c, k, d in ((32, 5, 2), (32, 3, 1), (64, 5, 1), (64, 5, 2), (64, 3, 1), (64, 3, 2)):
        add("", c, k, d, 2 * tiling(c, k, d, 1).T + 1, masks="none")
    # phase-split store: two geometries per kernel, an odd and an even row above T (the odd one reaches the zero-fill of the
    # odd phase's last item)
    # ("any" masks: under "strict" m2 is zero wherever m0 or m1 is, and within the halo of the row ends - the store's mask
    # multiply would hide the shortcut, the m1 multiply and the zeros outside the row)
    for (c, k, d), masks in (((32, 5, 1), "any"), ((32, 3, 2), "any"), ((64, 5, 2), "any"), ((64, 3, 1), "any")):
        T = tiling(c, k, d, 1).T
        odd = T + 1 if (T + 1) % 2 else T + 2
        add("", c, k, d, odd, masks=masks, store="psplit")
        add("", c, k, d, odd + 1, masks=masks, store="psplit")
    # launch shapes (windows from the compute-unit count): three tiles a row, units no multiple of the grid
    add("launch3", 32, 5, 1, 2 * 124 + 1, launch=3.0)              # both image buffers reused, n_local 3 and 4
    add("launch3", 32, 3, 2, 2 * 124 + 1, launch=3.0, masks="strict")
    add("launch1", 64, 5, 2, 2 * 56 + 1, launch=1.4)               # n_local 1 and 2
    add("launch2", 64, 5, 2, 2 * 56 + 1, launch=2.4, masks="strict")   # 2 and 3
    for c, k, d in ((64, 5, 2), (64, 5, 1), (64, 3, 1), (64, 3, 2)):   # >= 6: both rings wrap, the carry in `advance`
        add("launch6", c, k, d, 2 * tiling(c, k, d, 1).T + 1, launch=6.0)
    # chunked forward: 5 windows in launch groups of 2, 2, 1 - bit for bit the unchunked one
    add("chunk", 32, 5, 2, 2 * 120 + 1, n_win=5, chunk=2)
    add("chunk", 64, 5, 2, 2 * 56 + 1, n_win=5, chunk=2)
    # programs the placement must leave layer by layer
    add("neg", 64, 5, 3, 100, neg="64 channels at dilation 3")
    add("neg", 32, 5, 9, 100, neg="halo 36 > 32")
    add("neg", 32, 7, 1, 100, neg="7 taps")
    add("neg-stride2", 32, 5, 1, 100, neg="stride-2 conv2")
    add("neg-bypass", 32, 5, 1, 100, neg="conv2 adds a bypass, not conv1's input")
    add("neg-erf", 32, 5, 1, 100, neg="erf-GELU", act=ACT_GELU_ERF)
    add("neg-relu", 64, 5, 2, 100, neg="ReLU", act=ACT_RELU)
    add("neg-nmd", 32, 5, 1, 100, neg="NMD tap on conv1")
    add("neg-reader", 64, 5, 2, 100, neg="a third op reads conv1's output")
    add("neg-inplace", 32, 5, 1, 250, neg="conv2 writes in place")     # (250: one row-tiled tile a row, no tile reads another's)
    # the range guard: block outputs beyond 65 000 (both kernels); only the intermediate beyond the f16 range (64 channels)
    add("guard-out", 32, 5, 1, 125, guard=True, gain2=3.0e5)
    add("guard-out", 64, 5, 2, 57, guard=True, gain2=3.0e5)
    add("guard-mid", 64, 5, 2, 57, guard=True, gain1=3.0e5, gain2=1.0e-5)
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out


#: why each negative case is not a fused block: the condition of resblock_second (jg_prepare.hip) it meets, as source text
_SUPPORTS = "!(jg_resblock_supports(A.cout, A.k, A.dilation) || jg_resblock64_supports(A.cout, A.k, A.dilation))"
NEG_RULES = {
    "64 channels at dilation 3": _SUPPORTS, "halo 36 > 32": _SUPPORTS, "7 taps": _SUPPORTS,
    "stride-2 conv2": "B.stride != 1",
    "conv2 adds a bypass, not conv1's input": "hb.add_slot != A.in_buf",
    "erf-GELU": "ha.act_kind != JG_ACT_GELU_TANH", "ReLU": "ha.act_kind != JG_ACT_GELU_TANH",
    "NMD tap on conv1": "ha.ep != JG_EP_ACT1",
    "a third op reads conv1's output": "if (ib == n && m->ops[j].kind == JG_OP_CONV && m->ops[j].in_buf == A.out_buf) ib = j; else ok = false;",
    "conv2 writes in place": "writer == ib",
}

CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
POSITIVE = [c for c in CASES if c.neg is None and not c.guard]
NEGATIVE = [c for c in CASES if c.neg is not None]
GUARD = [c for c in CASES if c.guard]


# ---- ids -----------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 3, 2, 7)         # (+ halo / 2 + 1, halo + 2: runs that reach across a whole halo)


def tile_edge_ids(l: int, T: int, halo: int, n_win: int = 12, vocab: int = VOCAB, seed: int = 5, grow: int = 1) -> np.ndarray:
    """(n_win, 6, l) ids: random valid codons with runs of id 0.  Every frame is a row of its own to the kernels, so runs are
    placed frame by frame.  ``grow``: the first-layer mask op (3 taps, "any") shrinks a run of N by this much at either end;
    runs are written that much longer, so that what is described here holds for m0, the block's input mask.  By window
    (index mod 12): 0 no N; 1 all N; 2 ragged - every frame ends inside the first tile; 3 the row start and the row end, run
    lengths 1 .. halo / 2 + 2; 4 - 11 masked runs that begin and that end at every position of [T - halo - 1, T + halo + 1]
    (the first tile border and everything that reaches across it) and of the same range around 2 T when the row has it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(1, vocab, (n_win, 6, l))
    pad = halo // 2

    def zero(w, f, a, b):                                  # m0 = 0 on [a, b] (inclusive)
        ids[w, f, max(a - grow, 0): min(b + grow, l - 1) + 1] = 0

    lengths = RUN_LENGTHS + (pad + 1, halo + 2)
    # the runs around the tile borders, first fit over the 48 rows of windows 4 - 11 (3 unmasked positions between two runs)
    want = [q for B in (T, 2 * T) if l > B - halo - 1 for q in range(max(B - halo - 1, 0), min(B + halo + 1, l - 1) + 1)]
    rows = [[] for _ in range(48)]
    ends = set()

    def place(j, candidates):                              # the first candidate run some row still has room for
        for a, b in candidates:
            for step in range(48):
                r = rows[(j + step) % 48]
                if all(b + 4 <= a2 or b2 + 4 <= a for a2, b2 in r):
                    r.append((a, b))
                    ends.add(b)
                    return
        raise AssertionError(f"tile_edge_ids: no row left for a run at {candidates[0]} (l {l}, T {T}, halo {halo})")

    for j, q in enumerate(want):                           # a run that begins at q: the length of its turn, else a shorter one
        turn = lengths[j % len(lengths)]
        place(j, [(q, q + n - 1) for n in (turn,) + RUN_LENGTHS if q + n - 1 <= l - 1] or [(q, l - 1)])
    for j, q in enumerate(want):                           # ... and one that ends at q, where none does yet
        if q not in ends:
            turn = lengths[(j + 3) % len(lengths)]
            place(j, [(q - n + 1, q) for n in (turn,) + RUN_LENGTHS if q - n + 1 >= 0] or [(0, q)])
    for w in range(n_win):
        role = w % 12
        if role == 1:
            ids[w] = 0
        elif role == 2:
            for f in range(6):
                ids[w, f, max(1, min(l, T) * (f + 2) // 8 - grow) if l > 1 else 0:] = 0
        elif role == 3:
            for f in range(6):
                zero(w, f, 0, min(f * (pad + 2) // 5, l - 1))                       # 1 .. pad + 2 positions
                zero(w, f, max(l - 1 - (5 - f) * (pad + 2) // 5, 0), l - 1)
        elif role >= 4:
            for f in range(6):
                for a, b in rows[(role - 4) * 6 + f]:
                    zero(w, f, a, b)
    return ids.astype(np.uint8)


# ---- programs ------------------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    prog: object
    feeder: int                     # the first-layer conv: writes the block input
    conv1: int
    conv2: int
    masks: list                     # op indices of the mask ops that write m0, m1, m2 (absent: none)
    readers: list                   # stride-2 readers of a phase-split store
    extra: list                     # further convs of a negative case (bypass, third reader), checked per op
    pool: int
    ids: np.ndarray = field(default=None, repr=False)


X, H, Y, R1, R2 = 0, 1, 2, 3, 4     # activation slots: block input, intermediate, block output, readers


def build(c: Case, n_win: int | None = None) -> Built:
    """The program of a case (see the module docstring) and its ids."""
    from jaeger_amd import _lib as L
    from jaeger_amd.program import Program
    w = _Writer(zlib.crc32(c.name.encode()))
    emb_off = w.blob.add(w.rng.standard_normal((VOCAB, EMB)).astype(np.float32))
    same = L.PAD_SAME
    C, k, d = c.c, c.k, c.d
    mode = {"any": L.MASK_ANY, "strict": L.MASK_STRICT, "none": L.MASK_ANY}[c.masks]
    masked = c.masks != "none"
    none = L.JG_BUF_NONE
    act = lambda: w.stage(L.ST_ACT, arg=c.act)                                  # noqa: E731
    masks, readers, extra = [], [], []
    masks.append(w.op(L.OP_MASK, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, padding=same))
    feeder = w.op(L.OP_CONV, in_buf=L.JG_BUF_IDS, out_buf=X, in_mask=L.JG_BUF_IDS, out_mask=0, k=3, cin=EMB, cout=C, padding=same,
                  w_off=w.kernel(3, EMB, C, 2.0), b_off=emb_off, stages=[w.bias(C), w.stage(L.ST_ACT, arg=ACT_GELU_TANH)])
    m0, m1, m2 = (0, 1, 2) if masked else (none, none, none)
    if masked:
        masks.append(w.op(L.OP_MASK, in_mask=0, out_mask=1, k=k, dilation=d, padding=same, mask_mode=mode))
    st1 = [w.bias(C), w.bn(C), act()]
    nmd = c.neg is not None and "NMD" in c.neg
    if nmd:
        st1.insert(1, w.stage(L.ST_NMD, arg=0))
    conv1 = w.op(L.OP_CONV, in_buf=X, out_buf=H, in_mask=m0, out_mask=m1, k=k, cin=C, cout=C, dilation=d, padding=same,
                 w_off=w.kernel(k, C, C, c.gain1), stages=st1)
    add_slot, stride2, out2 = X, 1, Y
    if c.neg is not None and ("bypass" in c.neg or "stride-2" in c.neg):
        stride2 = 2 if "stride-2" in c.neg else 1
        w.op(L.OP_MASK, in_mask=0, out_mask=3, k=1, stride=stride2, padding=same)
        extra.append(w.op(L.OP_CONV, in_buf=X, out_buf=R2, in_mask=0, out_mask=3, k=1, cin=C, cout=C, stride=stride2, padding=same,
                          w_off=w.kernel(1, C, C), stages=[w.bias(C)]))
        add_slot = R2
    if c.neg is not None and "third op" in c.neg:
        w.op(L.OP_MASK, in_mask=1, out_mask=3, k=5, padding=same)
        extra.append(w.op(L.OP_CONV, in_buf=H, out_buf=R2, in_mask=1, out_mask=3, k=5, cin=C, cout=64, padding=same,
                          w_off=w.kernel(5, C, 64), stages=[w.bias(64)]))
    if c.neg is not None and "in place" in c.neg:
        out2 = H
    if masked:
        masks.append(w.op(L.OP_MASK, in_mask=1, out_mask=2, k=k, stride=stride2, dilation=d, padding=same, mask_mode=mode))
    conv2 = w.op(L.OP_CONV, in_buf=H, out_buf=out2, in_mask=m1, out_mask=m2, k=k, cin=C, cout=C, stride=stride2, dilation=d,
                 padding=same, w_off=w.kernel(k, C, C, c.gain2), stages=[w.bias(C), w.bn(C), w.stage(L.ST_ADD, arg=add_slot), act()])
    finals = 0
    if nmd:
        w.op(L.OP_NMD_FINAL, in_buf=H, in_mask=m1, cout=C, arg=0, b_off=w.normal(C, 0.3), f0=1e-7, out_vec=L.VEC_NMD, vec_off=0)
        finals = 1
    if c.store == "f16s":
        pm = 3 if masked else none
        if masked:
            w.op(L.OP_MASK, in_mask=m2, out_mask=3, k=5, padding=same)
        w.op(L.OP_CONV, in_buf=out2, out_buf=R1, in_mask=m2, out_mask=pm, k=5, cin=C, cout=64, padding=same,
             w_off=w.kernel(5, C, 64), stages=[w.bias(64)])
    else:
        assert c.store == "psplit" and masked, c.name
        pm = 3
        w.op(L.OP_MASK, in_mask=2, out_mask=3, k=5, stride=2, padding=same)
        readers.append(w.op(L.OP_CONV, in_buf=Y, out_buf=R1, in_mask=2, out_mask=3, k=5, cin=C, cout=64, stride=2, padding=same,
                            w_off=w.kernel(5, C, 64), stages=[w.bias(64), w.stage(L.ST_ACT, arg=ACT_GELU_TANH)]))
        w.op(L.OP_MASK, in_mask=2, out_mask=4, k=1, stride=2, padding=same)
        readers.append(w.op(L.OP_CONV, in_buf=Y, out_buf=R2, in_mask=2, out_mask=4, k=1, cin=C, cout=64, stride=2, padding=same,
                            w_off=w.kernel(1, C, 64), stages=[w.bias(64)]))
    pool = w.op(L.OP_POOL, in_buf=R1, in_mask=pm, cout=64, arg=L.POOL_AVG, out_vec=L.VEC_EMBEDDING)
    w.op(L.OP_DENSE, in_vec=L.VEC_EMBEDDING, out_vec=L.VEC_PREDICTION, cin=64, cout=2,
         w_off=w.blob.add((w.rng.standard_normal((64, 2)) * 0.1).astype(np.float32)), b_off=w.normal(2, 0.1))
    prog = Program(w.ops, w.blob.finish(), VOCAB, 2, False, finals * C, 64)
    t = c.til
    ids = tile_edge_ids(c.l, t.T, t.halo, n_win=n_win or c.n_win)
    return Built(prog, feeder, conv1, conv2, masks, readers, extra, pool, ids)


# ---- the block in float64, and the mutations the check must catch -------------------------------------------------------------
MUTATIONS = ("shortcut_m0", "no_m1", "outside", "shift", "no_m2")


def block_masks(prog, b: Built, masks: dict, shape) -> tuple:
    """(m0, m1, m2) as float64 (rows, frames, L) from a {slot: mask} dict - ones where the block carries no mask."""
    op1, op2 = prog.ops[b.conv1], prog.ops[b.conv2]
    get = lambda s: np.ones(shape) if s < 0 else np.asarray(masks[s], np.float64)     # noqa: E731
    return get(op1.in_mask), get(op2.in_mask), get(op2.out_mask)


def shift_tile(c: Case) -> int | None:
    """The tile the ``shift`` mutation moves by one position: the second one when it holds two positions or more."""
    t = c.til
    if c.l < 2:
        return None
    return 1 if t.tiles > 1 and min(c.l, 2 * t.T) - t.T >= 2 else 0


def block_ref(prog, b: Built, c: Case, x: np.ndarray, masks: dict, mutate: str | None = None) -> np.ndarray:
    """The block output in float64 from its input ``x`` (rows, frames, L, C) and the mask slots, written the way the kernels
    tile it: conv1 on the row extended by ``pad`` positions at either end (zeros outside the row), the intermediate times
    m1 and zero outside the row, conv2 over it, the shortcut, the GELU; a phase-split store times m2.  ``mutate``: one of
    MUTATIONS - the shortcut from x m0; the intermediate not multiplied by m1; not zeroed outside the row; one tile's outputs
    shifted by one position; the phase-split output not multiplied by m2."""
    from oracle import ops
    op1, op2 = prog.ops[b.conv1], prog.ops[b.conv2]
    t = c.til
    x = np.asarray(x, np.float64)
    l = x.shape[-2]
    m0, m1, m2 = block_masks(prog, b, masks, x.shape[:-1])
    st = ops.State(np.zeros(x.shape[:-1], np.uint8), mask={s: np.asarray(v) for s, v in masks.items()})
    y1 = ops.shifted_sum(x * m0[..., None], ops.conv_weights(prog, op1), 1, c.d, 2 * t.pad, l + 2 * t.pad)
    st1 = ops.State(st.ids)                                # (conv1's stages read no mask: bias, bn, GELU)
    h, _, _ = ops._stages(prog, _no_mask(op1), y1, np.zeros_like(y1), st1)
    m1e = np.zeros(x.shape[:-2] + (l + 2 * t.pad,))
    m1e[..., t.pad:t.pad + l] = 1.0 if mutate == "no_m1" else m1
    if mutate == "outside":
        m1e[..., :t.pad] = 1.0
        m1e[..., t.pad + l:] = 1.0
    y2 = ops.shifted_sum(h * m1e[..., None], ops.conv_weights(prog, op2), 1, c.d, 0, l)
    st.act[X] = x * m0[..., None] if mutate == "shortcut_m0" else x
    out, _, _ = ops._stages(prog, op2, y2, np.zeros_like(y2), st)
    if c.store == "psplit" and mutate != "no_m2":
        out = out * m2[..., None]
    if mutate == "shift":
        tile = shift_tile(c)
        lo, hi = tile * t.T, min((tile + 1) * t.T, l)
        out = out.copy()
        out[..., lo:hi - 1, :] = out[..., lo + 1:hi, :]
    return out


def _no_mask(op):
    new = type(op).from_buffer_copy(bytes(op))
    new.out_mask = -1
    return new


def chain_ref(prog, b: Built, c: Case, x: np.ndarray, masks: dict):
    """The block through oracle/ops.py, conv by conv (as test_gpu_op_taps._fused_block_ref): (output, magnitude); the
    phase-split store's mask multiplied in."""
    from oracle import ops
    op1, op2 = prog.ops[b.conv1], prog.ops[b.conv2]
    st = ops.State(np.zeros(np.asarray(x).shape[:-1], np.uint8), mask={s: np.asarray(v) for s, v in masks.items()})
    st.act[op1.in_buf] = np.asarray(x, np.float64)
    r1 = ops.run_op(prog, b.conv1, st)
    st.act[op2.in_buf] = r1.out
    st.M[op2.in_buf] = r1.M
    r2 = ops.run_op(prog, b.conv2, st)
    out, M = r2.out, r2.M
    if c.store == "psplit":
        m2 = block_masks(prog, b, masks, out.shape[:-1])[2][..., None]
        out, M = out * m2, M * m2
    return out, M


def emulate_block(prog, b: Built, c: Case, x: np.ndarray, masks: dict) -> np.ndarray:
    """The fused arithmetic: conv1 in split-f16 with its f32 epilogue, re-split to F16S (the LDS intermediate), conv2 the same
    way with the shortcut from the F16S block input, re-split (op_cases.emulate_conv twice)."""
    import op_cases as oc
    from oracle import ops
    op1, op2 = prog.ops[b.conv1], prog.ops[b.conv2]
    st = ops.State(np.zeros(np.asarray(x).shape[:-1], np.uint8), mask={s: np.asarray(v) for s, v in masks.items()})
    st.act[op1.in_buf] = np.asarray(x, np.float64)
    st.act[op2.in_buf] = oc.emulate_conv(prog, b.conv1, st)
    out = oc.emulate_conv(prog, b.conv2, st)
    if c.store == "psplit":
        out = out * block_masks(prog, b, masks, out.shape[:-1])[2][..., None]
    return out


def host_inputs(prog, b: Built):
    """The block input (rounded to what an F16S tensor holds) and the mask slots, chained from the ids in float64."""
    import op_cases as oc
    from oracle import ops
    st = ops.State(ops.program_rows(prog, b.ids))
    for i in range(b.conv1):
        ops.apply(prog, i, st, ops.run_op(prog, i, st))
    for i in b.masks[1:]:
        ops.apply(prog, i, st, ops.run_op(prog, i, st))
    x = oc.resplit(st.act[X].astype(np.float32)).astype(np.float64)
    return x, dict(st.mask)


# ---- the coverage census -------------------------------------------------------------------------------------------------------
CLASSES = ("tile_first", "tile_last", "row_end_inside", "row_end_own_tile", "hbm_shortcut", "hbm_at_tile_first",
           "hbm_at_tile_last", "m0_1_m1_0", "m1_0", "outside_intermediate", "tile_without_hbm", "tile_with_hbm", "m2_0",
           "odd_row_end")


def census(c: Case, m0: np.ndarray, m1: np.ndarray, m2: np.ndarray) -> dict:
    """Output positions (tiles for the two tile classes) of each class, from the masks (rows, frames, L) alone."""
    t = c.til
    l = c.l
    rows = m0.shape[0] * m0.shape[1]
    firsts = [q * t.T for q in range(t.tiles)]
    lasts = [q * t.T + t.T - 1 for q in range(t.tiles) if q * t.T + t.T - 1 < l]
    psplit = c.store == "psplit"
    vis = (m2 != 0) if psplit else np.ones(m0.shape, bool)      # (a phase-split store shows only outputs with m2 set)
    hbm = (m0 == 0) & vis                           # every position of the row is a live output
    with_hbm = sum(int(hbm[..., q * t.T:(q + 1) * t.T].any(axis=-1).sum()) for q in range(t.tiles))
    return {
        "tile_first": rows * len(firsts), "tile_last": rows * len(lasts),
        "row_end_inside": rows if (l - 1) % t.T != 0 else 0, "row_end_own_tile": rows if (l - 1) % t.T == 0 else 0,
        "hbm_shortcut": int(hbm.sum()), "hbm_at_tile_first": int(hbm[..., firsts].sum()),
        "hbm_at_tile_last": int(hbm[..., lasts].sum()) if lasts else 0,
        "m0_1_m1_0": int(((m0 != 0) & (m1 == 0) & vis).sum()), "m1_0": int((m1 == 0).sum()),
        "outside_intermediate": rows * 2 * t.pad,
        "tile_without_hbm": rows * t.tiles - with_hbm, "tile_with_hbm": with_hbm,
        "m2_0": int((m2 == 0).sum()) if psplit else 0, "odd_row_end": rows if psplit and l % 2 else 0,
    }


def required_classes(c: Case) -> set:
    """The classes the shape and mask form of a case can contain - each must be counted at least once."""
    t = c.til
    need = {"tile_first", "outside_intermediate", "row_end_inside" if (c.l - 1) % t.T else "row_end_own_tile"}
    if c.l >= t.T:
        need.add("tile_last")
    if c.masks != "none":
        need |= {"hbm_shortcut", "hbm_at_tile_first", "m1_0", "tile_with_hbm", "tile_without_hbm"}
        if c.l >= t.T:
            need.add("hbm_at_tile_last")
        if c.masks == "strict":
            need.add("m0_1_m1_0")
        if c.store == "psplit":
            need.add("m2_0")
    else:
        need.add("tile_without_hbm")
    if c.store == "psplit" and c.l % 2:
        need.add("odd_row_end")
    return need


def required_mutations(c: Case, counts: dict) -> list:
    """The mutations a case can show: those whose positions its census counts."""
    out = ["outside"]
    if counts["hbm_shortcut"]:
        out.append("shortcut_m0")
    if counts["m1_0"]:
        out.append("no_m1")
    if shift_tile(c) is not None:
        out.append("shift")
    if counts["m2_0"]:
        out.append("no_m2")
    return out
