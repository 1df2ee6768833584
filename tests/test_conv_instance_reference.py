"""CPU tier of the split-f16 conv instance census (tests/conv_instance_cases.py; the GPU tier is
tests/test_gpu_conv_instances.py).

(a) Source-text pins.  The switch tables at the bottom of jg_conv_f16_impl.h, the part selection of jg_launch_conv_f16 and the
    three has_*_pattern lists of jg_conv_f16.hip are parsed: each host list equals the pattern set of the tables it guards,
    and the census, its Python restatement of the dispatch and the library's own (jg_conv_inst.hip, what
    JG_MSTAT_TAP_INSTANCE reports) name exactly the instance set the tables compile.  Editing a JG_CASE line or a list entry
    without touching the census fails here.
(b) Every case compiles: jg_model_create's checks aside (GPU tier), oracle/ops.py evaluates every op of its program, the
    restated placement gives the target the instance the case is there for, and the split-f16 emulation of the target stays
    4x inside the bounds of op_cases.check on the case's own inputs.
(c) Every stage of every case is observable on the case's weights and inputs: the float64 reference with one epilogue stage
    dropped, with a DyT's gamma / beta swapped between two channels, or with an NMD tap read on the other side of a
    neighbouring stage leaves the bounds by at least 8x - so a dispatch to the wrong pattern cannot pass the GPU check.
"""
import copy
import re
from pathlib import Path

import numpy as np
import pytest

import conv_instance_cases as cc
import op_cases as oc

CSRC = Path(__file__).resolve().parents[1] / "jaeger_amd" / "csrc"
EMU_MARGIN = 4.0
MUT_MARGIN = 8.0


def _norm(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return " ".join(text.replace("\\\n", " ").split())


@pytest.fixture(scope="module")
def ep_values():
    text = (CSRC / "jg_common.h").read_text()
    vals = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (JG_EP_\w+) (0x[0-9a-f]+)u", text)}
    assert vals["JG_EP_NMD1"] == cc.N1 and vals["JG_EP_NORM1_AFF"] == cc.AFF1 and vals["JG_EP_NORM1_DYT"] == cc.DYT1
    assert vals["JG_EP_ADD"] == cc.ADD and vals["JG_EP_ACT1"] == cc.A1 and vals["JG_EP_NMD2"] == cc.N2
    assert vals["JG_EP_NORM2_AFF"] == cc.AFF2 and vals["JG_EP_NORM2_DYT"] == cc.DYT2 and vals["JG_EP_ACT2"] == cc.A2
    assert vals["JG_EP_RUNTIME"] == cc.RT
    return vals


def _ep(expr: str, vals: dict) -> int:
    """A pattern expression of the sources (``JG_EP_ADD | JG_EP_ACT1``, ``0u``) as a number."""
    expr = expr.strip().strip("()").strip()
    if expr in ("0u", "0"):
        return 0
    v = 0
    for name in expr.split("|"):
        v |= vals[name.strip()]
    return v


def _case_lists(block: str, vals: dict):
    """(patterns of the JG_CASE lines, patterns of the JG_CASE_HOT lines) of one switch, in order."""
    plain = [_ep(m.group(1), vals) for m in re.finditer(r"\bJG_CASE\(((?:0u|JG_EP_[\w |]+))\)", block)]
    hot = [_ep(m.group(1), vals) for m in re.finditer(r"\bJG_CASE_HOT\((JG_EP_[\w |]+)\)", block)]
    return plain, hot


@pytest.fixture(scope="module")
def compiled(ep_values):
    """The instance set the switch tables of jg_conv_f16_impl.h compile, from its text."""
    raw = (CSRC / "jg_conv_f16_impl.h").read_text()
    text = _norm(raw)
    inst = set()
    # -- JG_ROW_CASES(K): one `case` per pattern; the hot ones go through launch_hot (k = 5: the tanh build beside the general one)
    body = text[text.index("#define JG_ROW_CASES(K)"):text.index("} #if JG_CONV_PART == 1")]
    row, row_hot = [], []
    chunks = body.split(" case ")[1:]
    assert ["default: break;" in ch for ch in chunks] == [False] * (len(chunks) - 1) + [True]
    for chunk in chunks:
        m = re.match(r"(0u|\((JG_EP_[\w |]+)\)):", chunk)
        assert m, chunk[:80]
        ep = _ep(m.group(1), ep_values)
        launched = {_ep(x, ep_values) for x in re.findall(r"launch_(?:ke|hot)<K, \(?(0u|JG_EP_[\w |]+)\)?[,>]", chunk)}
        assert launched == {ep}, (cc.ep_name(ep), launched)
        row.append(ep)
        if "launch_hot<" in chunk:
            assert "if (K == 5 && a.act_kind == JG_ACT_GELU_TANH)" in chunk
            row_hot.append(ep)
    assert "template <int K, unsigned EP, bool FLAT> int launch_hot(" in text
    assert "return launch_ke<5, EP, FLAT, 128, true>(e, a, s); } else { return launch_ke<K, EP, FLAT>(e, a, s); }" in text
    tail = text[text.index("} #if JG_CONV_PART == 1"):]
    blocks = re.split(r"#(?:if|elif) JG_CONV_PART ", tail)[1:]
    assert [b.split(" ")[0] + " " + b.split(" ")[1] for b in blocks[:5]] == ["== 1", "== 2", "== 3", "== 4", ">= 5"], [b[:12] for b in blocks]
    p1, p2, p3, p4, p57 = blocks[:5]
    assert "jg_conv_f16_part_k5(jg_engine *e, const ConvHArgs &a, hipStream_t s) { JG_ROW_CASES(5) }" in p1
    assert "if (a.k == 7) { JG_ROW_CASES(7) } { JG_ROW_CASES(9) }" in p2
    for ep in row:
        inst |= {cc.Instance(1, 5, ep, False, 128, False), cc.Instance(2, 7, ep, False, 128, False), cc.Instance(2, 9, ep, False, 128, False)}
    inst |= {cc.Instance(1, 5, ep, False, 128, True) for ep in row_hot}
    # -- part 3: the window-packed table
    assert "#define JG_CASE(ep) case (ep): return launch_ke<5, (ep), true>(e, a, s);" in p3
    assert ("#define JG_CASE_HOT(ep) case (ep): return a.act_kind == JG_ACT_GELU_TANH ? launch_hot<5, (ep), true>(e, a, s) : "
            "launch_ke<5, (ep), true>(e, a, s);") in p3
    flat, flat_hot = _case_lists(p3, ep_values)
    inst |= {cc.Instance(3, 5, ep, True, 128, False) for ep in flat + flat_hot}
    inst |= {cc.Instance(3, 5, ep, True, 128, True) for ep in flat_hot}
    # -- part 4: launch_lut (in front of the tables)
    assert "jg_conv_f16_part_lut(jg_engine *e, const ConvHArgs &a, hipStream_t s) { return launch_lut(e, a, s); }" in p4
    lut_body = text[text.index("int launch_lut(jg_engine *e"):text.index("#define JG_ROW_CASES(K)")]
    assert ("#define JG_CASE(ep) case (ep): return a.cout == 128 ? launch_lut_e<(ep), 128>(e, a, s) : "
            "launch_lut_e<(ep), 129>(e, a, s);") in lut_body
    lut, _ = _case_lists(lut_body, ep_values)
    explicit = re.findall(r"launch_lut_e<\((JG_EP_[\w |]+)\), (\d+)(, true)?>", lut_body)
    assert len(explicit) == 3 and {e[1:] for e in explicit} == {("128", ", true"), ("128", ""), ("129", "")}, explicit
    for expr, cw, tanh in explicit:
        inst.add(cc.Instance(4, 0, _ep(expr, ep_values), False, int(cw), bool(tanh)))
    assert "if (a.cout == 128 && a.act_kind == JG_ACT_GELU_TANH) return launch_lut_e<" in lut_body
    for ep in lut:
        inst |= {cc.Instance(4, 0, ep, False, 128, False), cc.Instance(4, 0, ep, False, 129, False)}
    # -- parts 5 - 7 and 8 - 13: the run-time-geometry tables
    for part, cw in ((5, 64), (6, 32)):
        assert f"#if JG_CONV_PART == {part} #define JG_NARROW_CW {cw}" in tail or f"#elif JG_CONV_PART == {part} #define JG_NARROW_CW {cw}" in tail
    assert "#else #define JG_NARROW_CW 129 int jg_conv_f16_part_g128(" in tail
    assert ("#define JG_CASE(ep) case (ep): return a.flat ? launch_ke<5, (ep), true, JG_NARROW_CW>(e, a, s) : "
            "launch_ke<5, (ep), false, JG_NARROW_CW>(e, a, s);") in tail
    p813 = next(b for b in blocks if b.startswith(">= 8 && JG_CONV_PART <= 13"))
    p57 = tail[tail.index("int jg_conv_f16_part_g128("):tail.index("#elif JG_CONV_PART >= 8")]
    geom5, _ = _case_lists(p57, ep_values)
    for part, (k, cw) in cc.GEOM_PARTS.items():
        if k == 5:
            inst |= {cc.Instance(part, 5, ep, fl, cw, False) for ep in geom5 for fl in (False, True)}
    assert "#define JG_X_CW (((JG_CONV_PART - 8) % 3) == 0 ? 64 : ((JG_CONV_PART - 8) % 3) == 1 ? 32 : 129)" in p813
    assert "#define JG_X_K ((JG_CONV_PART - 8) / 3 == 0 ? 7 : 9)" in p813
    assert "#define JG_CASE(ep) case (ep): return launch_ke<JG_X_K, (ep), false, JG_X_CW>(e, a, s);" in p813
    geomx, _ = _case_lists(p813, ep_values)
    for part in range(8, 14):
        k, cw = (7 if (part - 8) // 3 == 0 else 9), (64, 32, 129)[(part - 8) % 3]
        assert cc.GEOM_PARTS[part] == (k, cw)
        inst |= {cc.Instance(part, k, ep, False, cw, False) for ep in geomx}
    # -- no instantiation site besides the ones read above (the pipelined build is JG_EXPERIMENT only)
    assert raw.count("launch_ke<") == 29 and raw.count("launch_lut_e<") == 5 and raw.count("launch_hot<") == 4, \
        (raw.count("launch_ke<"), raw.count("launch_lut_e<"), raw.count("launch_hot<"))
    assert "#ifdef JG_EXPERIMENT /* (the pipelined" not in text       # (comments are stripped: the guard itself is checked next)
    assert ("#ifdef JG_EXPERIMENT if (e->conv_pc == 2 && a.dil == 3 && a.cc_in % 2 == 0 && a.dbg == 0) return "
            "launch_ke<5, EP, FLAT, 128, true, true>(e, a, s); #endif") in text
    return {"all": inst, "row": row, "row_hot": row_hot, "flat": flat + flat_hot, "flat_hot": flat_hot, "lut": lut + [_ep(explicit[0][0], ep_values)],
            "geom5": geom5, "geomx": geomx}


def test_every_translation_unit_is_one_part():
    mk = (CSRC / "Makefile").read_text()
    units = re.search(r"^CONV\s*:=\s*(.*)$", mk, re.M).group(1).split()
    parts = sorted(int(re.search(r"#define JG_CONV_PART (\d+)", (CSRC / u).read_text()).group(1)) for u in units)
    assert parts == list(range(1, 14)), parts
    assert "jg_conv_inst.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "jg_conv_pc.hip" in re.search(r"^EXP_ONLY\s*:=\s*(.*)$", mk, re.M).group(1).split()


def test_census_names_exactly_the_compiled_instances(compiled):
    inst = compiled["all"]
    assert inst == cc.compiled_instances(), (sorted(inst - cc.compiled_instances()), sorted(cc.compiled_instances() - inst))
    assert compiled["row"] == list(cc.ROW) and compiled["row_hot"] == list(cc.HOT)
    assert set(compiled["flat"]) == set(cc.FLAT) and compiled["flat_hot"] == list(cc.HOT)
    assert set(compiled["lut"]) == set(cc.LUT) and compiled["geom5"] == list(cc.GEOM) and compiled["geomx"] == list(cc.GEOM)
    assert cc.instances_per_part() == {1: 24, 2: 42, 3: 17, 4: 19, 5: 30, 6: 30, 7: 30, 8: 15, 9: 15, 10: 15, 11: 15, 12: 15, 13: 15}
    assert len(inst) == 282
    covered = {c.want for c in cc.CASES if c.want is not None}
    assert covered | set(cc.UNREACHABLE) == inst and not covered & set(cc.UNREACHABLE), \
        (sorted(inst - covered - set(cc.UNREACHABLE)), sorted(covered - inst))
    assert len(cc.UNREACHABLE) == 18
    for dead, (rule, lands) in cc.UNREACHABLE.items():
        assert "jg_prepare.hip" in rule and lands in inst and lands not in cc.UNREACHABLE
        assert any(c.proves == dead and c.want == lands for c in cc.CASES), dead


def test_host_pattern_lists_equal_the_tables_they_guard(compiled, ep_values):
    text = _norm((CSRC / "jg_conv_f16.hip").read_text())
    lists = {m.group(1): [_ep(x, ep_values) for x in m.group(2).split(",")]
             for m in re.finditer(r"const unsigned (\w+)\[\] = \{(.*?)\};", text)}
    assert set(lists) == {"lut", "all", "flat", "nar"}
    for name, table in (("all", compiled["row"]), ("flat", compiled["flat"]), ("lut", compiled["lut"])):
        assert len(set(lists[name])) == len(lists[name]) and set(lists[name]) == set(table), \
            (name, [cc.ep_name(e) for e in set(lists[name]) ^ set(table)])
    assert set(lists["nar"]) == set(compiled["geom5"]) == set(compiled["geomx"]) and len(lists["nar"]) == len(compiled["geom5"])
    # which list guards what: the matcher and the tiling rule
    prep = _norm((CSRC / "jg_prepare.hip").read_text())
    assert "if (conv_ok && !jg_conv_f16_has_pattern(hp.ep, op.in_buf == JG_BUF_IDS)) {" in prep
    assert ("if (conv_ok && op.in_buf != JG_BUF_IDS && (op.cout != 128 || op.stride != 1 || hp.as_k5) && "
            "!jg_conv_f16_has_narrow_pattern(hp.ep))") in prep
    run = _norm((CSRC / "jg_run.hip").read_text())
    assert ("((op.cout == 128 && !hp.as_k5 && hp.ps_read == 0 && !hp.ps_store) ? jg_conv_f16_has_flat_pattern(hp.ep) : "
            "jg_conv_f16_has_narrow_pattern(hp.ep)) && (int64_t)nw * wp < (1 << 24) && flat_tiles * 100 <= row_tiles * 95") in run


def test_part_selection_of_the_launcher_and_its_restatements(compiled, ep_values):
    text = _norm((CSRC / "jg_conv_f16.hip").read_text())
    body = text[text.index("int jg_launch_conv_f16("):]
    pieces = ["if (a.lut != nullptr) {", "return jg_conv_f16_part_lut(e, a, s); }",
              "if (a.cw != HN) { if (a.k == 5) return a.cw == 64 ? jg_conv_f16_part_n64(e, a, s) : jg_conv_f16_part_n32(e, a, s);",
              "if (a.k == 7) return a.cw == 64 ? jg_conv_f16_part_x8(e, a, s) : jg_conv_f16_part_x9(e, a, s);",
              "return a.cw == 64 ? jg_conv_f16_part_x11(e, a, s) : jg_conv_f16_part_x12(e, a, s); }",
              "if (a.cout != HN || a.ostride != 1 || a.tap_lo != 0 || a.tap_hi != a.k - 1 || a.psplit) {",
              "if (a.k == 5) return jg_conv_f16_part_g128(e, a, s);",
              "return a.k == 7 ? jg_conv_f16_part_x10(e, a, s) : jg_conv_f16_part_x13(e, a, s); }",
              "if (a.flat) {", "return jg_conv_f16_part_flat(e, a, s); }",
              "if (a.k == 5) return jg_conv_f16_part_k5(e, a, s); return jg_conv_f16_part_k79(e, a, s);"]
    at = 0
    for p in pieces:
        assert p in body[at:], p
        at = body.index(p, at) + len(p)
    assert "constexpr int HM = 256, HN = 128," in text
    # the library's restatement (what JG_MSTAT_TAP_INSTANCE reports): the same tables, the same order of questions
    inst = _norm((CSRC / "jg_conv_inst.hip").read_text())
    sets = {m.group(1): (m.group(2) == "true", [_ep(x, ep_values) for x in m.group(3).split(",") if x.strip()])
            for m in re.finditer(r"const PatternSet (\w+) = \{(true|false), \{(.*?)\}\};", inst)}
    for name, table in (("ROW", cc.ROW), ("FLAT", cc.FLAT), ("LUT", cc.LUT), ("GEOM", cc.GEOM)):
        plain, eps = sets[name]
        assert 0 not in eps and len(set(eps)) == len(eps) and set(eps) | ({0} if plain else set()) == set(table), name
    hot = re.search(r"const unsigned HOT\[\] = \{(.*?)\};", inst).group(1)
    assert [_ep(x, ep_values) for x in hot.split(",") if x.strip()] == list(cc.HOT)
    assert _ep(re.search(r"const unsigned HOT_LUT = (.*?);", inst).group(1), ep_values) == cc.HOT_LUT
    at = 0
    for p in ["if (a.lut != nullptr) {", "if (a.cout != 128) return pack(4, 0, a.ep, false, 129, false, a.ep_rt);",
              "return pack(4, 0, a.ep, false, 128, a.ep == HOT_LUT && tanh_act, a.ep_rt);", "if (a.cw != 128) {",
              "const int part = a.k == 5 ? (a.cw == 64 ? 5 : 6) : a.k == 7 ? (a.cw == 64 ? 8 : 9) : (a.cw == 64 ? 11 : 12);",
              "if (a.cout != 128 || a.ostride != 1 || a.tap_lo != 0 || a.tap_hi != a.k - 1 || a.psplit) {",
              "return pack(a.k == 5 ? 7 : a.k == 7 ? 10 : 13, a.k, a.ep, a.flat != 0, 129, false, a.ep_rt);",
              "for (unsigned q : HOT) hot |= a.k == 5 && q == a.ep && tanh_act;", "if (a.flat) {",
              "return pack(3, 5, a.ep, true, 128, hot, a.ep_rt);", "return pack(a.k == 5 ? 1 : 2, a.k, a.ep, false, 128, hot, a.ep_rt);"]:
        assert p in inst[at:], p
        at = inst.index(p, at) + len(p)
    # the Python restatement maps onto the compiled set and reaches all of it
    image = set()
    for lut in (False, True):
        for k in (5, 7, 9):
            for cw, cout in ((128, 128), (128, 96), (64, 64), (32, 32)):
                for flat in (False, True):
                    for ep in set(cc.ROW) | set(cc.GEOM):
                        for act in (cc.ACT_GELU_TANH, cc.ACT_GELU_ERF):
                            got = cc.dispatch(lut=lut, k=k, cw=cw, cout=cout, ostride=1, tap_lo=0, tap_hi=k - 1, psplit=False,
                                              flat=flat, ep=ep, act=act)
                            if got is not None:
                                image.add(got)
    assert image == compiled["all"], sorted(image ^ compiled["all"])


def test_activation_kinds_and_forms_of_the_census():
    by_inst = {}
    for c in cc.CASES:
        by_inst.setdefault(c.want, []).append(c)
    for inst in cc.compiled_instances() - set(cc.UNREACHABLE):
        cases = by_inst[inst]
        beside_hot = not inst.tanh and ((inst.part in (1, 3) and inst.k == 5 and inst.ep in cc.HOT) or
                                        (inst.part == 4 and inst.cw == 128 and inst.ep == cc.HOT_LUT))
        acts = {c.act for c in cases}
        if beside_hot:                       # (the tanh-GELU goes to the hot build beside it)
            assert {cc.ACT_GELU_ERF, cc.ACT_RELU} <= acts and cc.ACT_GELU_TANH not in acts, inst
        else:
            assert cc.ACT_GELU_TANH in acts, inst
    for part in range(1, 14):
        mine = [c for c in cc.CASES if c.want is not None and c.want.part == part]
        assert {cc.ACT_GELU_ERF, cc.ACT_RELU} <= {c.act for c in mine if c.bits & cc.A1}, part
        assert any(c.store == "free" for c in mine), part
        rt = [c for c in mine if c.want.ep == cc.RT]
        assert any(c.ep_rt & cc.N1 and c.ep_rt & cc.N2 for c in rt) and any(not (c.ep_rt & cc.N1 and c.ep_rt & cc.N2) for c in rt), part
    assert sum(c.want is None for c in cc.CASES) == 2 and sum(c.mixed for c in cc.CASES) == 1
    assert {c.cout for c in cc.CASES if c.want is not None and c.want.cw == 129 and c.want.part != 4} >= {96, 128, 256}
    for part in cc.GEOM_PARTS:              # stride 2 on every part that takes it (the run-time-geometry tiles), by identity
        assert any(c.stride == 2 and c.want is not None and c.want.part == part for c in cc.CASES), part
    assert all(c.want.part in cc.GEOM_PARTS and not c.want.flat for c in cc.CASES if c.stride == 2)
    assert sum(c.store == "psplit" for c in cc.CASES) == 3
    assert all(4 <= c.n_win <= 6 for c in cc.CASES)


# ---- per-case checks ---------------------------------------------------------------------------------------------------------
def _worst(got, ref, M, gamma=oc.GAMMA):
    """op_cases.check's element criterion alone - max err / bound - without its table of offenders (a sort per call)."""
    return float((np.abs(got - ref) / (gamma * M + oc.REL * np.abs(ref) + oc.FLOOR)).max())


def _copy_op(op):
    return type(op).from_buffer_copy(bytes(op))


def _without(op, q):
    new = _copy_op(op)
    for s in range(q, op.n_stages - 1):
        new.stages[s] = op.stages[s + 1]
    new.n_stages = op.n_stages - 1
    return new


def _swapped(op, q):
    new = _copy_op(op)
    new.stages[q], new.stages[q + 1] = op.stages[q + 1], op.stages[q]
    return new


def _nmd_vectors(prog, built, state, taps, taps_m):
    from oracle import ops
    st = ops.State(state.ids, mask=dict(state.mask))
    st.part.update(taps)
    st.part_M.update(taps_m)
    res = [ops.run_op(prog, i, st) for i, _ in built.finals]
    return np.concatenate([r.out for r in res], axis=1), np.concatenate([r.M for r in res], axis=1)


def nmd_bounds(n_pos: int) -> tuple:
    """(gamma, RMS bound) of an NMD vector: the mean of n_pos tap values, each within op_cases.GAMMA x its magnitude of the
    float64 value (the conv's own bound), summed in f32 in any order (n 2^-24; RMS (sqrt n + 1) 2^-24, head_cases.gamma_sum)."""
    return oc.GAMMA + n_pos * 2.0 ** -24, oc.RMS_BOUND + (n_pos ** 0.5 + 1.0) * 2.0 ** -24


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_compiles_emulates_and_shows_every_stage(name):
    from oracle import ops
    c = cc.BY_NAME[name]
    # the restated placement and dispatch: the case selects its instance (and its tiling) by its own geometry
    if c.mixed:
        other = c.want._replace(part=1, flat=False)
        assert [cc.expected_instance(c, nw) for nw in (2, 2, 1)] == [c.want, c.want, other]
    else:
        assert cc.expected_instance(c) == c.want, (cc.expected_instance(c), c.want)
    b = cc.build(c)
    prog, op = b.prog, b.prog.ops[b.target]
    # every op evaluates (oracle/ops.py), one pass; the target's linear part once, its stage list and the mutations on it
    state = ops.State(ops.program_rows(prog, b.ids))
    for i in range(len(prog.ops)):
        if i == b.target:
            before = ops.State(state.ids, dict(state.act), dict(state.mask), dict(state.part), dict(state.vec))
            x = ops.conv_input(prog, op, state)
            wgt = ops.conv_weights(prog, op)
            lo, pl = ops.conv_geometry(x.shape[-2], op.k, op.stride, op.dilation, op.padding)
            y = ops.shifted_sum(x, wgt, op.stride, op.dilation, pl, lo)
            M0 = ops.shifted_sum(np.abs(x), np.abs(wgt), op.stride, op.dilation, pl, lo)
            base, base_m, (taps, taps_m) = ops._stages(prog, op, y, M0, state)
            ref = ops.OpOut(base, base_m, taps=taps, taps_M=taps_m)
            ops.apply(prog, i, state, ref)
        else:
            ops.apply(prog, i, state, ops.run_op(prog, i, state))
    assert set(state.vec) >= {ops.VEC_EMBEDDING, ops.VEC_PREDICTION} | ({ops.VEC_NMD} if b.finals else set())
    assert prog.ops[b.target - 1].kind == ops.OP_MASK and prog.ops[b.target - 1].out_mask == op.out_mask
    state = before                                                # (what the target read: the mask it writes under included)
    assert op.out_mask in state.mask
    emu = oc.emulate_conv(prog, b.target, state)
    res = oc.check(emu, ref.out, ref.M, f16s=True)
    assert res.worst * EMU_MARGIN <= 1.0 and res.rms * EMU_MARGIN <= oc.RMS_BOUND, res.report(f"{name} emulation")
    n_pos = base.shape[1] * base.shape[2]
    if b.finals:
        nmd_ref, nmd_m = _nmd_vectors(prog, b, state, taps, taps_m)
    kinds = [op.stages[q].kind for q in range(op.n_stages)]
    assert kinds[0] == ops.ST_BIAS
    for q in range(1, op.n_stages):
        if kinds[q] in (ops.ST_BN, ops.ST_DYT, ops.ST_ADD, ops.ST_ACT):
            mut, _, _ = ops._stages(prog, _without(op, q), y, M0, state)
            worst = _worst(mut, ref.out, ref.M)
            assert worst >= MUT_MARGIN, f"{name}: dropping stage {q} (kind {kinds[q]}) moves no element {MUT_MARGIN}x out: {worst:.3g}"
        if kinds[q] == ops.ST_DYT:
            p2 = copy.copy(prog)
            p2.blob = prog.blob.copy()
            g, be = op.stages[q].p2, op.stages[q].p3
            for off in (g, be):
                p2.blob[[off + 3, off + 4]] = prog.blob[[off + 4, off + 3]]
            mut, _, _ = ops._stages(p2, op, y, M0, state)
            worst = _worst(mut, ref.out, ref.M)
            assert worst >= MUT_MARGIN, f"{name}: DyT gamma / beta swapped between channels 3 and 4 moves nothing: {worst:.3g}"
        if kinds[q] == ops.ST_NMD:
            gamma, _ = nmd_bounds(n_pos)
            for other in (q - 1, q):                              # the tap read in front of the stage before it / behind the next
                if other + 1 >= op.n_stages:
                    continue
                _, _, (t2, tm2) = ops._stages(prog, _swapped(op, other), y, M0, state)
                got, _ = _nmd_vectors(prog, b, state, t2, tm2)
                worst = _worst(got, nmd_ref, nmd_m, gamma)
                assert worst >= MUT_MARGIN, f"{name}: NMD tap of stage {q} moved across stage {other if other < q else q + 1}: {worst:.3g}"
