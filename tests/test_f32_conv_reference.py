"""CPU tier of the exact-f32 conv and layer-norm checks (cases: tests/f32_conv_cases.py; GPU tier: tests/test_gpu_f32_conv.py).

(a) The launcher, pinned.  ``f32_conv_cases.tile_of`` / ``passes_of`` / ``tiles_m`` / ``lds_bytes`` restate ``jg_launch_conv``,
    ``conv_f32_cchunk``, ``jg_conv_tile_m`` and ``conv_f32_lds``; the tests here hold them to the source text and to the pass
    table of DESIGN 3.3.  ``jg_conv_tile_m`` cannot return 128: the three 128-position instantiations of ``jg_launch_conv``
    (``<2,2,2,2>``, ``<2,2,2,1>``, ``<4,1,1,1>``) are compiled and unreachable.  Whoever changes the tile choice meets
    ``test_tile_m_is_64_and_the_128_position_instantiations_are_dead`` and owes this census 128-position cases.
(b) The emulation.  ``emulate_conv`` is ``conv_f32_kernel`` in numpy float32 as its source states it: channel passes
    outermost, then the tap, then the 8-channel group of the pass, four rank-2 steps per group accumulated in f32 (each step
    one float32 product of a (positions, 2) by a (2, cout_pad) matrix added to the accumulator - the MFMA's own order inside a
    rank-2 step is not stated anywhere and is not modelled); both operands zero-padded to ``cin_pad`` / ``cout_pad``; every
    tile computed over all of its 64 positions; the epilogue stage by stage, rounded to f32 after each stage (the float64
    stage of oracle/ops.py on f32 values); the NMD partials per (row, tile) summed in f32 and finished in f32.
    ``emulate_ln`` is ``layernorm_kernel`` the same way: the sum over the channels in f32, the mean, the centred squares,
    ``sqrt`` in f32, the divide, the affine, the mask; the NMD partial row of tile 0, zeros in the others.
(c) The bounds are ``op_cases.check`` with ``GAMMA``, ``RMS_BOUND``, ``REL`` and ``FLOOR`` unchanged, on every case: the
    longest contraction here (k 5 x 512 channels = 2 560 terms) leaves the emulation as far inside as the shortest, so no case
    takes the ``GAMMA + n 2^-24`` form (measured: see the table ``test_emulation_margin_table`` prints; worst err / bound
    of a conv case 0.06, of a layer-norm case 0.05 with its RMS at 0.12 of RMS_BOUND).  An NMD vector is held to ``nmd_bounds`` of
    tests/test_conv_instance_reference.py (GAMMA plus the f32 sum over the positions).  The emulation sits at least 4 x inside
    on every case; every mutation lies at least 8 x outside on at least one case, and the test prints which.
(d) One mutation of the issue's list has no observable form: "the mask applied to the output but not the input" of the layer
    norm.  The mask is 0 or 1; where it is 1 both forms compute the same, where it is 0 both store 0 (finite inputs), and the
    NMD tap behind it multiplies by the same mask.  ``test_ln_mask_on_the_output_alone_is_not_observable`` shows the two forms
    bit-identical in the emulation on every case instead of pretending a bound could tell them apart.
(e) The census: which (BN, gridDim.y, partial column block, cin % 8, passes, partial last pass, tiles per row) the exact-f32
    legs of tests/test_gpu_op_taps.py and the golden projects reach, and that the new cases reach every cell those leave out.
(f) The plan refuses what the kernels do not cover (a conv or norm width that is no multiple of 4, a layer norm above 512
    channels), and every golden project still compiles to the program and blob recorded in golden/program_digests.json.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import f32_conv_cases as fc
import op_cases as oc
from test_conv_instance_reference import _copy_op, _norm, nmd_bounds

CSRC = Path(__file__).resolve().parents[1] / "jaeger_amd" / "csrc"
GOLDEN = Path(__file__).resolve().parent / "golden"
EMU_MARGIN = 4.0
MUT_MARGIN = 8.0
F = np.float32


# ---- (a) the launcher, pinned ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels_text():
    return _norm((CSRC / "jg_kernels.hip").read_text())


def test_tile_m_is_64_and_the_128_position_instantiations_are_dead(kernels_text):
    """jg_conv_tile_m returns 64 whatever it is given, so bm64 is always true in jg_launch_conv.  If this fails the tile choice
    has changed: the census of f32_conv_cases.py then owes cases on the 128-position instantiations."""
    assert "int jg_conv_tile_m(int l_out) { (void)l_out; return 64; }" in kernels_text
    assert ("int jg_conv_tile_m_for(int l_out, int k, int cin, int stride, int dil) { const int cin_pad = (cin + 7) / 8 * 8; "
            "if (conv_f32_lds(128, 128, k, cin_pad, stride, dil) > 160 * 1024) return 64; return jg_conv_tile_m(l_out); }") in kernels_text
    assert fc.TILE_M == 64 and [fc.tiles_m(l) for l in (1, 63, 64, 65, 128, 129, 165)] == [1, 1, 1, 2, 2, 3, 3]
    run = _norm((CSRC / "jg_run.hip").read_text())
    assert "static int f32_tiles(int L) { return (L + jg_conv_tile_m(L) - 1) / jg_conv_tile_m(L); }" in run
    assert "const int tm = jg_conv_tile_m_for(lo, op.k, op.cin, op.stride, op.dilation); a.tiles_m = (lo + tm - 1) / tm;" in run


def test_instantiation_ladder_of_the_launcher(kernels_text):
    body = kernels_text[kernels_text.index("int jg_launch_conv(jg_engine *e, const ConvArgs &a, hipStream_t s)"):]
    body = body[:body.index("__global__")]
    pieces = ["const bool bm64 = jg_conv_tile_m_for(a.L_out, a.k, a.cin, a.stride, a.dil) == 64;",
              "#else if (a.cout_pad % 128 == 0) return bm64 ? launch_conv_t<2, 2, 1, 2>(a, s) : launch_conv_t<2, 2, 2, 2>(a, s); #endif",
              "if (a.cout_pad % 64 == 0) return bm64 ? launch_conv_t<2, 2, 1, 1>(a, s) : launch_conv_t<2, 2, 2, 1>(a, s);",
              "return bm64 ? launch_conv_t<2, 1, 1, 1>(a, s) : launch_conv_t<4, 1, 1, 1>(a, s); }"]
    at = 0
    for p in pieces:
        assert p in body[at:], p
        at = body.index(p, at) + len(p)
    assert "#define JG_F32_SHAPE 0" in body
    assert "constexpr int BM = WM * TM * 32, BN = WN * TN * 32;" in kernels_text
    assert "dim3 grid((unsigned)((size_t)a.rows * a.tiles_m), (unsigned)((a.cout + BN - 1) / BN));" in kernels_text
    run = _norm((CSRC / "jg_run.hip").read_text())
    assert "a.cin = op.cin; a.cin_pad = (op.cin + 7) / 8 * 8; a.cout = op.cout; a.cout_pad = (op.cout + 31) / 32 * 32;" in run
    # WN x TN x 32 columns: <2,2,1,2> 128, <2,2,1,1> 64, <2,1,1,1> 32
    for cout, want in ((4, (32, 1)), (28, (32, 1)), (72, (32, 3)), (160, (32, 5)), (36, (64, 1)), (164, (64, 3)), (192, (64, 3)),
                       (100, (128, 1)), (228, (128, 2)), (384, (128, 3))):
        assert fc.tile_of(cout) == want, cout
    for bn, couts in fc.COUTS.items():
        assert all(fc.tile_of(c)[0] == bn for c in couts)
    assert {fc.instantiation(c) for c in (32, 64, 128)} == {"<2,1,1,1>", "<2,2,1,1>", "<2,2,1,2>"}


def test_pass_rule_and_lds_size(kernels_text):
    assert ("static int conv_f32_cchunk(int bm, int k, int cin_pad, int stride, int dil) { const size_t rows_in = (size_t)(bm - 1) * stride "
            "+ (size_t)(k - 1) * dil + 1; const long fit = (long)((160 * 1024) / (rows_in * sizeof(float))) - 4; if (fit >= cin_pad) "
            "return cin_pad; return fit < 8 ? 0 : (int)(fit / 8 * 8); }") in kernels_text
    assert ("static size_t conv_f32_lds(int bm, int bn, int k, int cch, int stride, int dil) { const size_t rows_in = (size_t)(bm - 1) * "
            "stride + (size_t)(k - 1) * dil + 1; const size_t lds_a = rows_in * (cch + 4) * sizeof(float), lds_c = (size_t)bm * (bn + 4) * "
            "sizeof(float); return ((lds_a > lds_c ? lds_a : lds_c) + 15) & ~(size_t)15; }") in kernels_text
    assert "b.cchunk = conv_f32_cchunk(BM, a.k, a.cin_pad, a.stride, a.dil);" in kernels_text
    assert "for (int c0 = 0; c0 < a.cin_pad; c0 += cch) { const int cw = min(cch, a.cin_pad - c0);" in kernels_text
    assert "const int gpass = cw >> 3, g0 = c0 >> 3;" in kernels_text
    # the table of the issue / DESIGN 3.3
    table = {(256, 7, 8, 2): (175, [224, 32]), (512, 5, 4, 1): (80, [504, 8]), (256, 9, 12, 1): (160, [248, 8]),
             (128, 15, 18, 1): (316, [120, 8]), (260, 9, 12, 1): (160, [248, 16])}
    assert {r[:4] for r in fc.PASS_ROWS} == set(table)
    for (cin, k, dil, stride), (rows, passes) in table.items():
        assert fc.rows_in(k, stride, dil) == rows and fc.passes_of(k, stride, dil, cin) == passes
        d1 = fc.one_pass_dilation(cin, k, dil, stride)
        assert len(fc.passes_of(k, stride, d1, cin)) == 1 and len(fc.passes_of(k, stride, d1 + 1, cin)) == 2
    # what the named models stage: one pass
    assert fc.rows_in(5, 1, 8) == 96 and fc.passes_of(5, 1, 8, 256) == [256]          # pyramid
    assert fc.rows_in(9, 1, 8) == 128 and fc.passes_of(9, 1, 8, 256) == [256]         # pyramid_k9
    for c in fc.CASES:
        ps = fc.passes_of(c.k, c.stride, c.dil, c.cin)
        assert fc.lds_bytes(fc.tile_of(c.cout)[0], c.k, ps[0], c.stride, c.dil) <= fc.LDS_BYTES, c.name
        assert sum(ps) == -(-c.cin // 8) * 8 and all(p % 8 == 0 for p in ps)


def test_layernorm_slots_of_the_kernel(kernels_text):
    assert "__shared__ float4 red[4 * 64 * 2];" in kernels_text
    assert "for (int j = 0; j < 2; ++j) { const int q = lane + 64 * j;" in kernels_text
    assert "for (int j = 0; j < 2; ++j) red[(wid * 2 + j) * 64 + lane] = nmd_acc[j];" in kernels_text
    assert "for (int p = wid; p < L; p += 4) {" in kernels_text
    # the second quad slot runs above 256 channels, rows shorter than the four waves leave waves idle
    assert {c.c > 256 for c in fc.LN_CASES} == {True, False} and {c.l < 4 for c in fc.LN_CASES} == {True, False}


def test_the_case_axes_are_all_there():
    names = set(fc.BY_NAME)
    assert all(f"cout{c}-bn{bn}" in names for bn, cs in fc.COUTS.items() for c in cs)
    assert all(f"cin{c}" in names for c in fc.CINS) and {c % 8 for c in fc.CINS} == {0, 4}
    assert all(f"l{l}-bn{bn}" in names for l in fc.ROW_LENGTHS for bn in (32, 64, 128))
    assert all(fc.BY_NAME[f"l{l}-bn{bn}"].n_taps == 2 and fc.BY_NAME[f"l{l}-bn{bn}"].cout % bn for l in fc.ROW_LENGTHS for bn in (32, 64, 128))
    assert {c.k for c in fc.CASES} >= {1, 2, 3, 4, 5, 7, 9, 15} and {c.dil for c in fc.CASES} >= {1, 2, 3, 8}
    assert {c.stride for c in fc.CASES} == {1, 2, 3}
    assert any(c.padding == "valid" and c.l_out == 1 for c in fc.CASES) and any(c.padding == "valid" and c.dil > 1 and c.l_out > 1 for c in fc.CASES)
    first = [c for c in fc.CASES if c.first]
    assert {(c.cin, c.k, c.mask_from_ids) for c in first} == {(e, k, m) for e in (4, 8, 16, 64) for k in (3, 7) for m in (True, False)}
    assert {c.ep for c in fc.CASES} == {"bias", "bn_act", "dyt", "add_act", "nmd1", "nmd2"}
    assert {c.mask_mode for c in fc.CASES} == {fc.MASK_ANY, fc.MASK_MAJORITY, fc.MASK_STRICT} and any(not c.out_mask for c in fc.CASES)
    chunked = [c for c in fc.CASES if c.chunk]
    assert {fc.tile_of(c.cout)[0] for c in chunked} == {32, 64, 128} and any(len(fc.passes_of(c.k, c.stride, c.dil, c.cin)) > 1 for c in chunked)
    assert all(c.n_win == 5 and c.chunk == 2 for c in chunked)
    two = [c for c in fc.CASES if c.name.startswith("pass2-")]
    one = [c for c in fc.CASES if c.name.startswith("pass1-")]
    assert len(two) == len(one) == 5 and all(c.l_out == 65 for c in two + one)
    assert {(c.c, c.l) for c in fc.LN_CASES if c.is_ln} >= {(c, l) for c in fc.LN_WIDTHS for l in fc.LN_ROWS}
    ln = [c for c in fc.LN_CASES if c.is_ln]
    assert {(c.mask, c.use_masking) for c in ln} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c.kind for c in fc.LN_CASES} == {"ln", "ln_add_act", "ln_nmd", "bn_act", "dyt"}
    assert all(c.l == 165 for c in fc.LN_CASES if c.kind == "ln_nmd") and {c.c for c in fc.LN_CASES if c.kind == "ln_nmd"} == set(fc.LN_WIDTHS)
    assert {c.c for c in fc.LN_CASES if not c.is_ln} == {4, 260, 512}
    assert 140 <= len(fc.CASES) + len(fc.LN_CASES) <= 160, (len(fc.CASES), len(fc.LN_CASES))


# ---- (b) the emulation -------------------------------------------------------------------------------------------------------
class Ctx:
    """A case's program evaluated by the float64 reference up to its target: what the target reads, and its reference."""

    def __init__(self, built):
        from oracle import ops
        self.b, self.prog = built, built.prog
        self.op = self.prog.ops[built.target]
        state = ops.State(ops.program_rows(self.prog, built.ids))
        for i in range(built.target):
            ops.apply(self.prog, i, state, ops.run_op(self.prog, i, state))
        self.state = state
        self.ref = ops.run_op(self.prog, built.target, state)
        after = ops.State(state.ids, mask=dict(state.mask))
        after.part.update(self.ref.taps)
        after.part_M.update(self.ref.taps_M)
        self.nmd = [ops.run_op(self.prog, i, after) for i in built.finals]

    def out_mask(self, shape):
        from oracle import ops
        m = ops._mask_of(self.state, self.op.out_mask)
        return np.ones(shape, np.float64) if m is None else m


_CTX = {}


def ctx_of(name):
    if name not in _CTX:
        _CTX[name] = Ctx(fc.build(fc.BY_NAME[name]) if name in fc.BY_NAME else fc.build_ln(fc.LN_BY_NAME[name]))
    return _CTX[name]


def stages_f32(prog, op, v, state, first=0):
    """The stage list on f32 values, rounded to f32 after every stage; returns (result f32, {slot: tapped f32 tensor})."""
    from oracle import ops
    v = np.asarray(v, F).astype(np.float64)
    zero = np.zeros(v.shape)
    taps = {}
    for s in range(first, op.n_stages):
        one = _copy_op(op)
        one.n_stages = s + 1
        v, _, (t, _) = ops._stages(prog, one, v, zero, state, first=s)
        v = v.astype(F).astype(np.float64)
        taps.update({k: a.astype(F) for k, a in t.items()})
    return v.astype(F), taps


def finish_nmd(prog, final_op, partial, mask):
    """nmd_final in f32: the partial rows of every (frame, tile) summed, over the count of valid positions plus epsilon, less
    the moving mean.  partial (rows, frames, tiles, C) f32, mask (rows, frames, L) or None."""
    s = partial.reshape(partial.shape[0], -1, partial.shape[-1]).sum(axis=1, dtype=F)
    n_pos = mask.shape[1] * mask.shape[2]
    cnt = F(n_pos) if final_op.in_mask < 0 else mask.reshape(mask.shape[0], -1).sum(axis=1).astype(F)[:, None] + F(final_op.f0)
    mm = np.asarray(prog.blob[final_op.b_off:final_op.b_off + final_op.cout], F)
    return (s / cnt - mm).astype(F)


def tile_partials(tap, mask, n_tiles, lost_from=None):
    """(rows, frames, tiles, C): the f32 sum of tap x mask over the 64 positions of every tile (``tap`` may run past L_out to
    the end of the last tile: the positions a broken bounds check would count)."""
    r, f, n, c = tap.shape
    v = tap * mask[..., None].astype(F)
    full = np.zeros((r, f, n_tiles * fc.TILE_M, c), F)
    full[:, :, :n] = v
    part = full.reshape(r, f, n_tiles, fc.TILE_M, c).sum(axis=3, dtype=F)
    if lost_from is not None:
        part[:, :, lost_from:] = 0
    return part


def emulate_conv(ctx, mut=None):
    """(output f32 (rows, frames, L_out, cout), [nmd vector f32 per finish]) of the case's target conv - see the module
    docstring - with mutation ``mut`` of the kernel."""
    from oracle import ops
    prog, op, state = ctx.prog, ctx.op, ctx.state
    rd = op
    if mut == "mask_from_ids_ignored":
        rd = _copy_op(op)
        rd.in_mask = ops.BUF_NONE
    x = ops.conv_input(prog, rd, state).astype(F)
    w = ops.conv_weights(prog, op).astype(F)
    k, cin, cout = w.shape
    cin_pad, cout_pad = -(-cin // 8) * 8, -(-cout // 32) * 32
    bn, gy = fc.tile_of(cout)
    l_in = x.shape[-2]
    l_out, pl = ops.conv_geometry(l_in, op.k, op.stride, op.dilation, op.padding)
    if mut == "even_k_mirrored":
        total = max((l_out - 1) * op.stride + (k - 1) * op.dilation + 1 - l_in, 0)
        pl = total - total // 2
    if mut == "stride_phase":
        pl -= 1
    n_tiles = fc.tiles_m(l_out)
    n_out = n_tiles * fc.TILE_M
    wp = np.zeros((k, cin_pad, gy * bn if gy * bn > cout_pad else cout_pad), F)
    wp[:, :cin, :cout] = w
    rows = x.shape[0] * x.shape[1]
    need = (n_out - 1) * op.stride + (k - 1) * op.dilation + 1
    left = max(pl, 0)
    xp = np.zeros((rows, left + max(l_in - min(pl, 0), need) + 1, cin_pad), F)
    xp[:, left:left + l_in, :cin] = x.reshape(rows, l_in, cin)
    shift = left - pl                                   # (a negative pad_left - the stride-phase mutation - reads one on)
    if mut == "pad_garbage":
        assert cin % 8 == 4
        xp[:, :, cin:] = 1.0
        wp[:, cin:, :cout] = 0.5
    if mut == "wrong_grid_block":
        assert gy >= 2
        wp[:, :, bn:2 * bn] = wp[:, :, :bn]
    passes = fc.passes_of(op.k, op.stride, op.dilation, cin)
    acc = np.zeros((rows * n_out, wp.shape[2]), F)
    c0 = 0
    for p, cw in enumerate(passes):
        if mut == "second_pass_dropped" and p > 0:
            break
        for t in range(k):
            a0 = t * op.dilation + shift
            xs = np.ascontiguousarray(xp[:, a0:a0 + (n_out - 1) * op.stride + 1:op.stride, c0:c0 + cw]).reshape(rows * n_out, cw)
            if mut == "tap_dropped_63_64" and t == 0:
                xs = xs.reshape(rows, n_out, cw).copy()
                xs[:, [q for q in (63, 64) if q < n_out]] = 0
                xs = xs.reshape(rows * n_out, cw)
            wbase = 0 if (mut == "g0_left_out" and p > 0) else c0
            for g in range(cw // 8):
                for step in range(4):
                    a = g * 8 + 2 * step
                    acc += xs[:, a:a + 2] @ wp[t, wbase + a:wbase + a + 2]
        c0 += cw
    acc = acc.reshape(x.shape[0], x.shape[1], n_out, -1)
    y, taps = stages_f32(prog, op, acc[:, :, :l_out, :cout], state)
    if mut == "upper_quads_written":
        extra = gy * bn - cout
        assert 0 < extra
        y = y.copy()
        flat = y.reshape(y.shape[0], -1)                # (the rows of a launch are one array: the store lands in the next position)
        n = min(extra, cout)
        idx = (np.arange(1, flat.shape[1] // cout)[:, None] * cout + np.arange(n)[None, :]).ravel()
        flat[:, idx] = 0.0                              # (zero weights, so a zero accumulator: whatever the stages make of it, not y)
    nmd = []
    if ctx.b.finals:
        om = ctx.out_mask(y.shape[:3])
        count_mask, tap_src = om, taps
        if mut == "nmd_counts_beyond_l_out":
            # the tail tile's positions at or beyond L_out: computed from zero rows, mask 1
            ext = acc[:, :, :, :cout]
            st2 = ops.State(state.ids, act=dict(state.act), mask=dict(state.mask))
            full_mask = np.ones(ext.shape[:3])
            full_mask[:, :, :l_out] = om
            if op.out_mask >= 0:
                st2.mask[op.out_mask] = full_mask
            _, tap_src = stages_f32(prog, op, ext, st2)
            count_mask = full_mask
        for q, i in enumerate(ctx.b.finals):
            fo = prog.ops[i]
            part = tile_partials(tap_src[fo.arg], count_mask, n_tiles, lost_from=1 if mut == "nmd_later_tiles_lost" else None)
            nmd.append(finish_nmd(prog, fo, part, om))
    return y, nmd


def emulate_ln(ctx, mut=None):
    """(output f32, [nmd vector]) of a layer-norm case's ELTWISE op as layernorm_kernel computes it."""
    from oracle import ops
    prog, op, state = ctx.prog, ctx.op, ctx.state
    x = np.asarray(state.act[op.in_buf], F)
    c = x.shape[-1]
    ln = op.stages[0]
    assert ln.kind == ops.ST_LN
    mk = ctx.out_mask(x.shape[:3]).astype(F)[..., None]
    lmk = mk if ln.arg else np.ones_like(mk)
    v = x if mut == "mask_on_output_only" else (x * lmk).astype(F)
    inv_c = F(1.0) / F(c)
    upto = 256 if mut == "mean_without_second_slot" else c
    mean = (v[..., :upto].sum(axis=-1, keepdims=True, dtype=F) * inv_c).astype(F)
    d = (v - mean).astype(F)
    upto = 256 if mut == "variance_without_second_slot" else c
    sq = (d[..., :upto] * d[..., :upto]).astype(F).sum(axis=-1, keepdims=True, dtype=F)
    denom = np.sqrt((sq * inv_c + F(ln.f0)).astype(F)).astype(F)
    ga, be = np.asarray(prog.blob[ln.p2:ln.p2 + c], F), np.asarray(prog.blob[ln.p3:ln.p3 + c], F)
    y = (((d / denom).astype(F) * ga).astype(F) + be).astype(F) * lmk
    y, taps = stages_f32(prog, op, y.astype(F), state, first=1)
    nmd = []
    n_tiles = fc.tiles_m(x.shape[2])
    for i in ctx.b.finals:
        fo = prog.ops[i]
        tap = taps[fo.arg]
        if mut == "nmd_slot0_for_slot1":
            tap = tap.copy()
            tap[..., 256:] = tap[..., :c - 256]
        row = (tap * mk).astype(F).sum(axis=2, dtype=F)                       # tile 0 carries the row's sums
        part = np.zeros(tap.shape[:2] + (n_tiles, c), F)
        part[:, :, 0] = row
        if mut == "later_tiles_not_zeroed":
            part[:, :, 1:] = 1.0
        nmd.append(finish_nmd(prog, fo, part, mk[..., 0]))
    return y, nmd


def worst_of(ctx, y, nmd):
    """(check result of the tensor, worst err / bound over the NMD vectors, worst NMD RMS / its bound)."""
    res = oc.check(y, ctx.ref.out, ctx.ref.M)
    n_pos = ctx.ref.out.shape[1] * ctx.ref.out.shape[2]
    gamma, rms_bound = nmd_bounds(n_pos)
    w_nmd = r_nmd = 0.0
    for got, r in zip(nmd, ctx.nmd):
        rr = oc.check(got[:, None, None, :], r.out[:, None, None, :], r.M[:, None, None, :], gamma=gamma)
        w_nmd, r_nmd = max(w_nmd, rr.worst), max(r_nmd, rr.rms / rms_bound)
    return res, w_nmd, r_nmd


_MARGINS = {}


@pytest.mark.parametrize("name", [c.name for c in fc.CASES] + [c.name for c in fc.LN_CASES])
def test_emulation_sits_inside_the_bounds(name):
    from oracle import ops
    ctx = ctx_of(name)
    prog = ctx.prog
    for i in range(len(prog.ops)):                       # every op of the program evaluates in the reference
        assert prog.ops[i].kind != ops.OP_STRANDS
    conv = name in fc.BY_NAME
    if conv:
        c = fc.BY_NAME[name]
        assert ctx.ref.out.shape[2:] == (c.l_out, c.cout) and ctx.ref.out.shape[0] == c.n_win
        assert len(ctx.b.finals) == c.n_taps
        y, nmd = emulate_conv(ctx)
    else:
        c = fc.LN_BY_NAME[name]
        assert ctx.ref.out.shape[2:] == (c.l, c.c)
        if not c.is_ln:                                  # a plain element-wise op: its stage list in f32
            y, _ = stages_f32(prog, ctx.op, np.asarray(ctx.state.act[ctx.op.in_buf], F), ctx.state)
            nmd = []
        else:
            y, nmd = emulate_ln(ctx)
    res, w_nmd, r_nmd = worst_of(ctx, y, nmd)
    _MARGINS[name] = (res.worst, res.rms / oc.RMS_BOUND, w_nmd, r_nmd)
    assert res.worst * EMU_MARGIN <= 1.0 and res.rms * EMU_MARGIN <= oc.RMS_BOUND, res.report(f"{name} emulation")
    assert w_nmd * EMU_MARGIN <= 1.0 and r_nmd * EMU_MARGIN <= 1.0, (name, w_nmd, r_nmd)
    # the inputs exercise the mask: some position of the target's output is masked and some is not (under a halo of more than
    # 8 positions the "any" rule leaves nothing masked: there the input mask alone varies)
    if ctx.op.out_mask >= 0 and ctx.ref.out.shape[2] > 2:
        om = ctx.out_mask(ctx.ref.out.shape[:3])
        assert (om != 0).any(), name
        assert (om == 0).any() or (conv and (c.k - 1) * c.dil > 8), name


def test_emulation_margin_table():
    """Runs behind the cases (in a narrower selection: over those that ran): the measured margins, worst first."""
    if not _MARGINS:
        pytest.skip("no case of this module was selected")
    for kind, names in (("conv", [n for n in _MARGINS if n in fc.BY_NAME]), ("layer norm / element-wise", [n for n in _MARGINS if n in fc.LN_BY_NAME])):
        if not names:
            continue
        rows = sorted(names, key=lambda n: -_MARGINS[n][0])
        print(f"\n{kind}: {len(names)} cases, emulation worst err/bound {max(_MARGINS[n][0] for n in names):.3g}, worst rms/bound "
              f"{max(_MARGINS[n][1] for n in names):.3g}, nmd worst err/bound {max(_MARGINS[n][2] for n in names):.3g} "
              f"(all must be <= {1 / EMU_MARGIN:.2f})")
        for n in rows[:5]:
            print("  %-44s err/bound %.3g  rms/bound %.3g  nmd err/bound %.3g  nmd rms/bound %.3g" % ((n,) + _MARGINS[n]))


# ---- (c) mutations -----------------------------------------------------------------------------------------------------------
PASS2 = [c.name for c in fc.CASES if c.name.startswith("pass2-")]
CONV_MUTATIONS = {
    "second_pass_dropped": PASS2,
    "g0_left_out": PASS2,
    "pad_garbage": ["cin12", "cin36", "cin260", "pass2-cin260-k9-d12-s1"],
    "upper_quads_written": ["cout28-bn32", "cout36-bn64", "cout100-bn128", "cout72-bn32", "cout164-bn64", "cout228-bn128"],
    "wrong_grid_block": ["cout72-bn32", "cout164-bn64", "cout228-bn128", "cout384-bn128"],
    "tap_dropped_63_64": ["l64-bn32", "l65-bn64", "l129-bn128", "cout32-bn32"],
    "even_k_mirrored": ["k2", "k4", "k4-dil3", "stride2-k4"],
    "stride_phase": ["stride2", "stride3", "stride3-k4", "valid-k4-stride2"],
    "mask_from_ids_ignored": ["first-e4-k3-idmask", "first-e8-k7-idmask", "first-e16-k3-idmask", "first-e64-k7-idmask"],
    "nmd_counts_beyond_l_out": ["l1-bn32", "l2-bn64", "l63-bn128", "l65-bn32", "l129-bn64", "l165-bn128"],
    "nmd_later_tiles_lost": ["l65-bn32", "l127-bn64", "l129-bn128", "l165-bn32", "pass2-cin512-k5-d4-s1"],
}
NMD_MUTATIONS = ("nmd_counts_beyond_l_out", "nmd_later_tiles_lost", "nmd_slot0_for_slot1", "later_tiles_not_zeroed")
LN_MUTATIONS = {
    "mean_without_second_slot": ["ln-c260-l5-", "ln-c384-l165-ln_nmd-mask-um", "ln-c512-l1-"],
    "variance_without_second_slot": ["ln-c260-l5-", "ln-c384-l165-ln_nmd-mask-um", "ln-c512-l1-"],
    "nmd_slot0_for_slot1": ["ln-c260-l165-ln_nmd-mask-um", "ln-c384-l165-ln_nmd-mask-um", "ln-c512-l165-ln_nmd-mask-um"],
    "later_tiles_not_zeroed": ["ln-c4-l165-ln_nmd-mask-um", "ln-c260-l165-ln_nmd-mask-um", "ln-c512-l165-ln_nmd-nomask-um"],
}


def _ln_name(prefix):
    """The one layer-norm case of a width and row length (its form rotates with the cross: named by prefix)."""
    hits = [c.name for c in fc.LN_CASES if c.name.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    return hits[0]


def _mutation_rows(table, emulate, resolve=lambda n: n):
    rows = []
    for mut, names in table.items():
        for n in names:
            ctx = ctx_of(resolve(n))
            y, nmd = emulate(ctx, mut)
            res, w_nmd, r_nmd = worst_of(ctx, y, nmd)
            by = max(w_nmd, r_nmd) if mut in NMD_MUTATIONS else max(res.worst, res.rms / oc.RMS_BOUND)
            rows.append((mut, resolve(n), by))
    return rows


def _assert_all_caught(rows):
    print()
    failures = []
    for mut in dict.fromkeys(r[0] for r in rows):
        mine = [r for r in rows if r[0] == mut]
        best = max(mine, key=lambda r: r[2])
        print(f"  {mut:30s} caught by {best[1]:36s} {best[2]:10.3g} x the bound   (" + ", ".join(f"{r[1]} {r[2]:.3g}" for r in mine) + ")")
        if best[2] < MUT_MARGIN:
            failures.append((mut, best))
    assert not failures, failures


def test_every_conv_mutation_is_caught():
    """Each mutation of conv_f32_kernel lies at least 8 x outside the bounds on at least one case (printed: which)."""
    assert all(n in fc.BY_NAME for names in CONV_MUTATIONS.values() for n in names)
    _assert_all_caught(_mutation_rows(CONV_MUTATIONS, emulate_conv))


def test_every_layernorm_mutation_is_caught():
    def resolve(n):
        return n if n in fc.LN_BY_NAME else _ln_name(n)
    _assert_all_caught(_mutation_rows(LN_MUTATIONS, emulate_ln, resolve))


def test_ln_mask_on_the_output_alone_is_not_observable():
    """Module docstring (d): with a 0 / 1 mask and finite inputs the two forms store the same bits, taps included."""
    n = 0
    for c in fc.LN_CASES:
        if not (c.is_ln and c.mask and c.use_masking):
            continue
        ctx = ctx_of(c.name)
        y0, nmd0 = emulate_ln(ctx)
        y1, nmd1 = emulate_ln(ctx, "mask_on_output_only")
        masked = ctx.out_mask(y0.shape[:3]) == 0
        n += int(masked.sum())
        np.testing.assert_array_equal(y0[masked], y1[masked], err_msg=c.name)
        np.testing.assert_array_equal(y0[~masked], y1[~masked], err_msg=c.name)
        for a, b in zip(nmd0, nmd1):
            np.testing.assert_array_equal(a, b, err_msg=c.name)
    assert n > 100


# ---- (e) the census ----------------------------------------------------------------------------------------------------------
#: the exact-f32 legs of tests/test_gpu_op_taps.py: op_cases model -> positions per row
F32_LEGS = {"brain": 500, "zeus_mixed": 500, "pyramid": 665, "pyramid_k7": 665, "pyramid_k9": 665, "baseline500": 500,
            "brain_ln": 500, "brain_majority": 500, "brain_strict": 500, "baseline500_dicodon_pos": 300}


def conv_cells(prog, l):
    """The census cell of every conv of ``prog`` at rows of ``l`` positions, and the widths of its layer norms."""
    from oracle import ops
    length = {}
    cells, ln_widths = set(), set()
    for op in prog.ops:
        l_in = l if op.in_buf == ops.BUF_IDS else length.get(op.in_buf, l)
        if op.kind == ops.OP_CONV:
            lo, _ = ops.conv_geometry(l_in, op.k, op.stride, op.dilation, op.padding)
            cells.add(fc.cell(op.cin, op.cout, op.k, op.stride, op.dilation, lo))
            length[op.out_buf] = lo
        elif op.kind == ops.OP_MAXPOOL1D:
            length[op.out_buf] = l_in // 2
        elif op.out_buf >= 0:
            length[op.out_buf] = l_in
            if op.kind == ops.OP_ELTWISE and op.n_stages and op.stages[0].kind == ops.ST_LN:
                ln_widths.add(op.cout)
    return cells, ln_widths


def _golden_programs():
    from conftest import load_model_cfg
    from jaeger_amd.plan import build_plan
    from jaeger_amd.program import compile_plan
    from jaeger_amd.weights import random_weights
    import warnings
    for path in sorted(GOLDEN.glob("*_project.yaml")):
        name = path.name[:-len("_project.yaml")]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plan = build_plan(load_model_cfg(name))
            yield name, compile_plan(plan, random_weights(plan, 38341))


def test_census_the_new_cases_reach_what_the_named_models_leave_out():
    from jaeger_amd import legacy
    reached, ln_reached = set(), set()
    for name, l in F32_LEGS.items():
        _, _, prog = oc.compile_model(name)
        cells, lnw = conv_cells(prog, l)
        reached |= cells
        ln_reached |= lnw
    reached |= conv_cells(legacy.compile_legacy(legacy.load_legacy_h5(GOLDEN / "legacy_data" / "models" / "default" / "WRes_1024.h5")), 665)[0]
    for name, prog in _golden_programs():
        if getattr(prog, "strands", 1) > 1:
            continue                                    # (the two-strand model runs as the table net)
        for l in (165, 500):                            # 500 and 1 500 bases
            cells, lnw = conv_cells(prog, l)
            reached |= cells
            ln_reached |= lnw
    mine = {c.cell for c in fc.CASES}
    axes = ("BN", "grid.y", "partial block", "cin % 8", "passes", "partial pass", "tiles")
    print("\ncensus cells (%s): existing exact-f32 legs and golden projects %d, new cases %d, new only %d" %
          (", ".join(axes), len(reached), len(mine), len(mine - reached)))
    for cell in sorted(reached | mine):
        print("  %-46s %s %s" % (cell, "models" if cell in reached else "      ", "cases" if cell in mine else ""))
    # what the named models leave out, which the cases must reach: no conv of theirs takes a second pass, the only partial
    # column block is a 16-wide conv's on BN 32, the only half group the 4-wide embedding's, the widest layer norm has 256
    assert {c[4] for c in reached} == {1}, "a named model takes channel passes: the census text of DESIGN is out of date"
    assert {c[0] for c in reached if c[2]} <= {32} and max(ln_reached) <= 256
    for bn in (32, 64, 128):
        assert any(c[0] == bn and c[2] for c in mine), bn                                  # every BN with a partial last block
        assert any(c[0] == bn and c[4] == 2 and c[5] for c in mine), bn                    # ... and under two passes, the last one partial
        assert {c[6] for c in mine if c[0] == bn} == {1, 2, 3}, bn                         # one, two, three tiles per row
        assert any(c[0] == bn and c[3] == 4 for c in mine), bn
    assert {c[1] for c in mine} >= {1, 2, 3, 5}
    assert any(c[3] == 4 and c[4] == 2 for c in mine)                                     # passes and channel padding together
    # every product of the axes the models leave out: (BN, partial block, passes)
    want = {(bn, part, passes) for bn in (32, 64, 128) for part in (False, True) for passes in (1, 2)}
    assert {(c[0], c[2], c[4]) for c in mine} >= want, sorted(want - {(c[0], c[2], c[4]) for c in mine})
    assert max(c.c for c in fc.LN_CASES) == 512 and {c.c for c in fc.LN_CASES if c.c > 256} >= {260, 384, 512}


# ---- (f) refusals and unchanged programs -------------------------------------------------------------------------------------
def _rep_cfg(layers):
    from conftest import load_model_cfg
    import copy
    cfg = copy.deepcopy(load_model_cfg("brain"))
    cfg["representation_learner"]["hidden_layers"] = layers
    cfg.pop("reliability_model", None)
    return cfg


def _conv(filters, **kw):
    return {"name": "masked_conv1d", "config": dict({"filters": filters, "kernel_size": 3, "padding": "same"}, **kw)}


@pytest.mark.parametrize("layers, word", [
    ([_conv(30)], r"rep/0: a conv of \d+ -> 30 channels \(both must be multiples of 4"),
    ([_conv(32), {"name": "residual_block", "config": {"filters": 30, "kernel_size": 3}}], r"conv1: a conv of 32 -> 30 channels"),
    ([_conv(516), {"name": "masked_layernorm", "config": {}}], r"rep/1: masked_layernorm over 516 channels \(up to 512"),
    ([_conv(512), {"name": "residual_block", "config": {"filters": 1024, "kernel_size": 3, "norm_type": "masked_layernorm"}}],
     r"bn1: masked_layernorm over 1024 channels \(up to 512"),
])
def test_plan_refuses_the_widths_the_kernels_do_not_cover(layers, word):
    from jaeger_amd import plan as P
    with pytest.raises(P.UnsupportedLayer, match=word):
        P.build_plan(_rep_cfg(layers))


def test_plan_takes_the_widths_at_the_limits():
    from jaeger_amd import plan as P
    P.build_plan(_rep_cfg([_conv(4), _conv(512), {"name": "masked_layernorm", "config": {}}, _conv(1024), {"name": "masked_batchnorm", "config": {}}]))
    text = (CSRC / "jg_model.hip").read_text()
    assert "static int validate_widths(const jg_model *m)" in text and "rc = validate_widths(m);" in text
    assert f"op.cout <= {P.LAYERNORM_MAX_CHANNELS}" in text and P.CHANNEL_QUAD == 4
    kern = _norm((CSRC / "jg_kernels.hip").read_text())          # the launch-time checks stay
    assert 'JG_REQUIRE(a.cin % 4 == 0 && a.cout % 4 == 0, JG_ERR_UNSUPPORTED, "conv: cin=%d / cout=%d must be multiples of 4", a.cin, a.cout);' in kern
    assert 'JG_REQUIRE(a.c % 4 == 0 && a.c <= 512, JG_ERR_UNSUPPORTED, "layernorm: c=%d must be a multiple of 4 up to 512", a.c);' in kern
    assert 'JG_REQUIRE(a.c % 4 == 0, JG_ERR_UNSUPPORTED, "eltwise: c=%d must be a multiple of 4", a.c);' in kern


def program_digest(prog) -> dict:
    return {"ops": hashlib.sha256(b"".join(bytes(op) for op in prog.ops)).hexdigest(), "n_ops": len(prog.ops),
            "blob": hashlib.sha256(np.ascontiguousarray(prog.blob, np.float32).tobytes()).hexdigest(), "blob_floats": int(prog.blob.size)}


def test_golden_projects_compile_to_the_recorded_programs():
    """golden/program_digests.json was recorded at the commit before the width refusals went into the plan: every golden
    project compiles to the same op bytes and the same weight blob (stand-in weights of seed 38341)."""
    import ctypes

    from jaeger_amd import _lib as L
    want = json.loads((GOLDEN / "program_digests.json").read_text())
    assert ctypes.sizeof(L.JgOp) == want["sizeof_jg_op"]
    got = {name: program_digest(prog) for name, prog in _golden_programs()}
    assert set(got) == set(want["projects"]) and len(got) >= 15
    for name in sorted(got):
        rec = want["projects"][name]                # (no blob digest where packing evaluates exp / sin: the file's note)
        assert {k: got[name][k] for k in rec} == rec and {"ops", "n_ops", "blob_floats"} <= set(rec), name
    assert sum("blob" in rec for rec in want["projects"].values()) >= 12
