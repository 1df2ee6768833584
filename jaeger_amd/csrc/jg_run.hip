// C-ABI of libjaeger_hip.so, forward part: where every op runs (jg_place_op), one launcher per placement, the op-program
// interpreter that sequences them (run_chunk) and jg_forward.  Host logic only - shapes come from jg_shape_walk.
#include <map>
#include <mutex>
#include <utility>

#include "jg_host.h"

bool jg_tab_mfma_row_fits(int L_out, int k, int dil);       // jg_tabnet.hip: the matrix-core form's id image holds the row

// ---- placement -------------------------------------------------------------------------------------------------------
static size_t small_conv0(const jg_model *m) { return m->ops[0].kind == JG_OP_CONV ? 0 : 1; }   // first conv of a small-window model

PlaceCtx jg_place_ctx(const jg_model *m, const std::vector<OpShape> *shp, int l) {
  PlaceCtx c{m->precision, m->e->fuse_resblock != 0, false, false};
  if (shp == nullptr) return c;
  // the 32-channel family: one fused kernel from ids to pooled sums when the rows fit its 160 positions; longer
  // rows of such a model run layer by layer (on the narrow split-f16 kernels - 3-tap convs as tap-masked 5-tap ones)
  if (c.prec == 1 && m->small != nullptr) {
    const int L0 = (*shp)[small_conv0(m)].L_out;
    c.small = L0 >= 1 && L0 <= jg_small_max_positions() && l <= 192;
  }
  // the table net: rows whose LDS image fits (else - rows too long - layer by layer)
  if (m->tab_conv >= 0) {
    const jg_op &t = m->ops[(size_t)m->tab_conv];
    c.tab = jg_tab_lds_bytes(t.k, m->tab_vocab, m->tab_cq, l, t.dilation) <= 160 * 1024;
  }
  return c;
}

// Where op i runs.  The whole-row kernels come first (they swallow ops of every kind), then the conv placements the
// preparation passes of jg_prepare.hip decided (ConvHPrep), then the pool a split-f16 conv reduced in its epilogue.
// Below a placement, three launchers still pick between two forms of the same kernel family, each from one field:
// launch_conv_f16 the table-lookup form of a first conv (hp.d_lut, else matrix cores), launch_tab_net the matrix-core
// form of the table net (m->tab_wfrag and the row fits, else the LDS table), launch_ordinary the F16S max pool (hp.pool_f16s).
Place jg_place_op(const jg_model *m, size_t i, const PlaceCtx &c) {
  const jg_op &op = m->ops[i];
  const ConvHPrep &hp = m->hprep[i];
  if (c.small && (int)i < m->small->pool_op) return op.kind == JG_OP_NMD_FINAL ? PL_SMALL_NMD : PL_SMALL_SKIP;
  if (c.tab && (int)i == m->tab_pool) return PL_TAB_POOL;
  if (c.tab && (int)i == m->tab_conv) return PL_TAB_CONV;
  if (c.small && (int)i == m->small->pool_op) return PL_SMALL_POOL;
  if (op.kind == JG_OP_CONV) {
    if (c.prec != 1 || !hp.f16_ok) return PL_CONV_F32;          // (f16_ok: a compiled tiling and epilogue pattern exist)
    if (c.fuse_rb && hp.rb_second >= 0) return PL_RB_CONV1;
    if (c.fuse_rb && hp.rb_first >= 0) return op.cout == 64 ? PL_RB64 : PL_RB32;
    return PL_CONV_F16;
  }
  if (jg_op_is_mixer(op.kind)) return PL_MIXER;
  if (op.kind == JG_OP_POOL && c.prec == 1 && m->pool_fused_by[i] >= 0) return PL_POOL_FUSED;
  return PL_ORDINARY;
}

// ---- the profiling bracket: two events around a launch, read out by jg_profile_read (jg_engine.hip) ------------------
static int prof_event(jg_engine *e, hipEvent_t *ev) {
  if (!e->pool.empty()) {
    *ev = e->pool.back();
    e->pool.pop_back();
    return JG_OK;
  }
  JG_HIP(hipEventCreate(ev));
  return JG_OK;
}

static int prof_begin(jg_engine *e, hipStream_t s, int cls, double flops, ProfEvent *pe) {
  if (!e->profile) return JG_OK;
  int rc;
  if ((rc = prof_event(e, &pe->a)) != JG_OK || (rc = prof_event(e, &pe->b)) != JG_OK) return rc;
  pe->flops = flops;
  pe->cls = cls;
  JG_HIP(hipEventRecord(pe->a, s));
  return JG_OK;
}

// rc = the launch's result, handed through; the events of a failed launch go back to the pool
static int prof_end(jg_engine *e, hipStream_t s, ProfEvent *pe, int rc) {
  if (!e->profile) return rc;
  if (rc != JG_OK) { e->pool.push_back(pe->a); e->pool.push_back(pe->b); return rc; }
  JG_HIP(hipEventRecord(pe->b, s));
  e->pending.push_back(*pe);
  return JG_OK;
}

static double conv_flops(const jg_op &op, const OpShape &r, int nw) {
  return 2.0 * op.k * op.cin * op.cout * (double)nw * r.in.frames * r.L_out;
}

// ---- JG_OPT_POISON_WORKSPACE (include/jaeger_hip.h lists the buffers and what is left alone) -------------------------
static int poison_fill(const jg_engine *e, void *p, int64_t bytes, hipStream_t s) {
  if (e->poison >= 0 && p != nullptr && bytes > 0) JG_HIP(hipMemsetAsync(p, e->poison, (size_t)bytes, s));
  return JG_OK;
}

// in front of a launch group's first launch, behind jg_ensure_workspace: every scratch buffer over its allocated capacity.
// Stream order puts the fill behind the previous group's output copies (copy_out queues them on the same stream).
static int poison_workspace(jg_model *m, hipStream_t s) {
  const jg_engine *e = m->e;
  if (e->poison < 0) return JG_OK;
  const int64_t f = (int64_t)sizeof(float);
  int rc = JG_OK;
  for (int i = 0; i < JG_MAX_BUFS && rc == JG_OK; ++i)
    if ((rc = poison_fill(e, m->act[i], m->act_cap[i] * f, s)) == JG_OK && (rc = poison_fill(e, m->msk[i], m->msk_cap[i], s)) == JG_OK)
      rc = poison_fill(e, m->nmd_part[i], m->nmd_cap[i] * f, s);
  for (int i = 0; i < JG_MAX_VECS && rc == JG_OK; ++i)
    if ((rc = poison_fill(e, m->vec[i], m->vec_cap[i] * f, s)) == JG_OK) rc = poison_fill(e, m->merged[i], m->merged_cap[i], s);
  if (rc == JG_OK) rc = poison_fill(e, m->cvt_scratch, m->cvt_cap * f, s);
  if (rc == JG_OK) rc = poison_fill(e, m->hy_scratch, m->hy_cap, s);
  if (rc == JG_OK) rc = poison_fill(e, m->pool_part, m->pool_part_cap * f, s);
  if (rc == JG_OK) rc = poison_fill(e, m->tap_buf, m->tap_cap, s);
  if (rc == JG_OK && m->small != nullptr) rc = poison_fill(e, m->small->d_part, m->small->part_cap, s);
  return rc;
}

// ---- launchers: (model, op index, the op's shape record, [ids], rows of the chunk, stream) ---------------------------
static void resolve_stages(const jg_model *m, const jg_op &op, StageArg *dst, int *n) {
  *n = op.n_stages;
  for (int s = 0; s < op.n_stages; ++s) {
    const jg_stage &st = op.stages[s];
    StageArg &g = dst[s];
    g.kind = st.kind;
    g.arg = st.arg;
    g.f0 = st.f0;
    g.pad_ = 0;
    auto wp = [&](int64_t off) -> const float * { return off >= 0 ? m->d_w + off : nullptr; };
    g.p0 = wp(st.p0); g.p1 = wp(st.p1); g.p2 = wp(st.p2); g.p3 = wp(st.p3);
    if (st.kind == JG_ST_ADD) g.p0 = m->act[st.arg];
    if (st.kind == JG_ST_NMD) g.p0 = m->nmd_part[st.arg];
  }
}

// the whole conv stack of a small-window model, ids to pooled channel sums (c0: the record of its first conv)
static int launch_small_net(jg_model *m, const OpShape &c0, const uint8_t *d_ids, int nw, hipStream_t s) {
  jg_engine *e = m->e;
  JgSmallNet *sn = m->small;
  const int64_t rows = (int64_t)nw * 6;
  const int64_t had = sn->part_cap;
  int rc = grow(&sn->d_part, &sn->part_cap, rows * sn->n_slots * JG_SMALL_PARTW * (int64_t)sizeof(float));
  if (rc != JG_OK || (sn->part_cap != had && (rc = poison_fill(e, sn->d_part, sn->part_cap, s)) != JG_OK)) return rc;
  static const int dbg = [] { const char *ev = jg_exp_env("JG_SMALL_DBG"); return ev ? atoi(ev) : 0; }();
  JgSmallArgs a;
  memset(&a, 0, sizeof(a));
  a.ids = d_ids; a.lut = sn->d_lut; a.wfrag = sn->d_wfrag; a.epi = sn->d_epi; a.part = sn->d_part;
  a.overflow = m->d_overflow;
  a.rows = rows; a.L = c0.in.L; a.L0 = c0.L_out; a.pad0 = c0.pad_left; a.vocab = m->vocab;
  a.use_mask = sn->use_mask; a.pool_kind = sn->pool_kind; a.n_slots = sn->n_slots;
  a.dbg = dbg;
  for (int q = 0; q < JG_SMALL_MAX_LAYERS; ++q) a.layer[q] = sn->layer[q];
  ProfEvent pe;
  if ((rc = prof_begin(e, s, JG_PROF_FUSED_SMALL, (sn->flops_per_pos0 + sn->flops_per_pos) * (double)rows * c0.L_out, &pe)) != JG_OK)
    return rc;
  return prof_end(e, s, &pe, jg_launch_small_net(e, a, sn->n_conv, sn->k0, s));
}

// NMD_FINAL in front of the small-window kernel's pool: finish the tap the kernel accumulated for this slot
static int launch_small_nmd(jg_model *m, size_t i, int nw, hipStream_t s) {
  const jg_op &op = m->ops[i];
  const JgSmallNet *sn = m->small;
  int tap = 0;
  for (int t = 1; t <= sn->n_taps; ++t)
    if (sn->tap_part_slot[t] == op.arg && sn->tap_conv_op[t] < (int)i) tap = t;
  return jg_launch_small_pool_final(sn->d_part, 6, sn->n_slots, tap, nw, 2, m->d_w + op.b_off, op.f0,
                                    m->vec[op.out_vec] + op.vec_off, m->vec_w[op.out_vec], s);
}

// layout conversions queued by the format plan in front of op i: into the scratch tensor, then the slot takes the
// scratch's place (same bytes per element in both layouts)
static int convert_layouts(jg_model *m, size_t i, const OpShape &r, int nw, hipStream_t s) {
  jg_engine *e = m->e;
  const ConvHPrep &hq = m->hprep[i];
  for (int q = 0; q < hq.n_cvt; ++q) {
    const int slot = hq.cvt_slot[q];
    const Shape &t = r.cvt[q];
    const int64_t rows = (int64_t)nw * t.frames;
    // (the conversion in front of a row mixer with a profiling class is timed as a class of its own: what a kernel
    // variant that reads F16S directly would save)
    const MixerKind *mk = jg_mixer_kind(m->ops[i].kind);
    const bool timed = e->profile && mk != nullptr && mk->prof_cvt >= 0;
    ProfEvent pe;
    int rc = timed ? prof_begin(e, s, mk->prof_cvt, 0.0, &pe) : JG_OK;
    if (rc != JG_OK) return rc;
    if (hq.cvt_to_f32[q]) rc = jg_launch_f16s_to_f32(reinterpret_cast<const uint4 *>(m->act[slot]), rows, t.L, t.C, m->cvt_scratch, s);
    else rc = jg_launch_f32_to_f16s(m->act[slot], rows, t.L, t.C, reinterpret_cast<uint4 *>(m->cvt_scratch), s, m->d_overflow);
    if (timed) rc = prof_end(e, s, &pe, rc);
    if (rc != JG_OK) return rc;
    std::swap(m->act[slot], m->cvt_scratch);
    std::swap(m->act_cap[slot], m->cvt_cap);
  }
  return JG_OK;
}

// the table net: conv on ids, bias / activation and the global pool behind it in one launch, into the pool's vector
static int launch_tab_net(jg_model *m, size_t i, const OpShape &r, const uint8_t *d_ids, int nw, hipStream_t s) {
  jg_engine *e = m->e;
  const jg_op &op = m->ops[i], &po = m->ops[(size_t)m->tab_pool];
  const int l = r.in.L, lo = r.L_out, pl = r.pad_left;
  JgTabArgs a;
  memset(&a, 0, sizeof(a));
  a.ids = d_ids; a.table = m->tab_table; a.bias = m->tab_bias;
  a.out = m->vec[po.out_vec] + po.vec_off; a.out_ld = m->vec_w[po.out_vec];
  a.rows = nw * m->id_frames; a.L = l; a.L_out = lo; a.pad_left = pl; a.k = op.k; a.dil = op.dilation;
  a.vocab = m->tab_vocab; a.zero_id = m->tab_zero; a.cout = op.cout; a.cq = m->tab_cq; a.act = m->tab_act; a.pool_kind = po.arg;
  JG_REQUIRE(m->id_frames == 1, JG_ERR_UNSUPPORTED, "table net: rows of one frame only");
  ProfEvent pe;
  int rc = prof_begin(e, s, JG_PROF_TABLE, 2.0 * op.k * op.cin * op.cout * (double)a.rows * lo, &pe);
  if (rc != JG_OK) return rc;
  if (m->tab_wfrag != nullptr && jg_tab_mfma_row_fits(lo, op.k, op.dilation) && !e->tab_lds_only) {
    JgTabMArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.ids = d_ids; ma.wfrag = m->tab_wfrag; ma.bias = m->tab_bias512; ma.out = a.out; ma.out_ld = a.out_ld;
    ma.rows = a.rows; ma.L = l; ma.L_out = lo; ma.pad_left = pl; ma.k = op.k; ma.dil = op.dilation; ma.cout = op.cout;
    ma.act = m->tab_act; ma.pool_kind = po.arg;
    rc = jg_launch_tab_mfma(e, ma, s);
  } else {
    rc = jg_launch_tab_conv_pool(e, a, s);
  }
  return prof_end(e, s, &pe, rc);
}

// conv2 of a fused residual block: its launch computes conv1 (op hp.rb_first) too (jg_resblock.hip; wide: the 64-channel
// kernel of jg_resblock64.hip, whose waves split into conv1 / conv2 roles)
static int launch_resblock(jg_model *m, size_t i, const OpShape &r, int nw, hipStream_t s, bool wide) {
  jg_engine *e = m->e;
  const jg_op &op = m->ops[i];
  const ConvHPrep &hp = m->hprep[i];
  const jg_op &first = m->ops[(size_t)hp.rb_first];
  JgResBlockArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.xh = reinterpret_cast<const uint4 *>(m->act[first.in_buf]);
  ra.y = reinterpret_cast<uint4 *>(m->act[op.out_buf]);
  ra.m0 = first.in_mask >= 0 ? m->msk[first.in_mask] : nullptr;
  ra.m1 = op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr;
  ra.m2 = op.out_mask >= 0 ? m->msk[op.out_mask] : nullptr;
  ra.wfrag = hp.d_rb_wfrag;
  ra.epi = hp.d_rb_epi;
  ra.overflow = m->d_overflow;
  ra.rows = nw * r.in.frames; ra.L = r.in.L; ra.k = op.k; ra.dil = op.dilation;
  if (wide) jg_resblock64_tiling(r.in.L, op.k, op.dilation, &ra.nb, &ra.tile_out, &ra.tiles_per_row);
  else jg_resblock_tiling(r.in.L, op.k, op.dilation, &ra.nb, &ra.tile_out, &ra.tiles_per_row);
  ra.psplit = hp.ps_store ? 1 : 0;
  ProfEvent pe;
  int rc = prof_begin(e, s, JG_PROF_MFMA_F16X3, conv_flops(op, r, nw) * 2.0, &pe);      // both convs of the block
  if (rc != JG_OK) return rc;
  return prof_end(e, s, &pe, wide ? jg_launch_resblock64(e, ra, s) : jg_launch_resblock(e, ra, s));
}

// ConvHArgs of a split-f16 conv from its preparation record and geometry: the tap range of a conv that rides the 5-tap
// kernel and the rewriting of a stride-2 conv on a phase-split input included; the tiling and pool_out are set by the caller
static void conv_f16_args(const jg_model *m, size_t i, const OpShape &r, const uint8_t *d_ids, int nw, ConvHArgs &a) {
  const jg_op &op = m->ops[i];
  const ConvHPrep &hp = m->hprep[i];
  memset(&a, 0, sizeof(a));
  a.xh = op.in_buf == JG_BUF_IDS ? nullptr : reinterpret_cast<const uint4 *>(m->act[op.in_buf]);
  a.ids = op.in_buf == JG_BUF_IDS ? d_ids : nullptr;
  a.embh = hp.d_embh;
  a.mask_from_ids = op.in_mask == JG_BUF_IDS;
  a.mask_in = op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr;
  a.mask_out = op.out_mask >= 0 ? m->msk[op.out_mask] : nullptr;
  a.wh = hp.d_wh;
  a.y = m->act[op.out_buf];
  a.overflow = m->d_overflow;
  a.rows = nw * r.in.frames;
  a.L_in = r.in.L; a.L_out = r.L_out;
  a.cc_in = hp.cc_in; a.cout = op.cout; a.cout_pad = op.cout;
  a.k = op.k; a.dil = op.dilation; a.pad_left = r.pad_left;
  a.tap_lo = 0; a.tap_hi = op.k - 1;
  if (hp.as_k5) {              // taps (5 - k) / 2 .. of five: the same input offsets when the left pad grows with them
    a.k = 5;
    a.dil = op.k == 1 ? 1 : op.dilation;
    a.tap_lo = std::max(1, (5 - op.k) / 2);      // >= 1: tap_lo != 0 is the kernel's "some taps are skipped" flag
    a.tap_hi = a.tap_lo + op.k - 1;
    a.pad_left = r.pad_left + a.tap_lo * a.dil;
  }
  a.cw = hp.cw;
  a.ostride = op.stride;
  a.cc_row = hp.cc_in;
  if (hp.ps_read != 0) {
    // the input was stored phase-split and masked by its writer (plan_phase_split): this stride-2 conv runs at
    // stride 1 over (L + 1) / 2 positions - five taps as three over the two phases, the 1x1 bypass on the even phase
    a.mask_in = nullptr;
    a.L_in = (r.in.L + 1) / 2;                       // == L_out (TF SAME at stride 2: ceil(L / 2))
    a.cc_row = 2 * hp.cc_in;
    a.k = 5; a.dil = 1; a.ostride = 1;
    if (hp.ps_read == 1) {
      a.cc_in = 2 * hp.cc_in;
      a.wh = hp.d_wh_ps[r.in.L & 1];
      a.tap_lo = 1; a.tap_hi = 3;
      a.pad_left = 1 + a.tap_lo * a.dil;           // a 3-tap SAME conv pads one position on the left
    } else {
      a.tap_lo = a.tap_hi = 2;
      a.pad_left = 0 + a.tap_lo * a.dil;
    }
  }
  a.psplit = hp.ps_store ? 1 : 0;
  a.L_res = a.ostride == 2 ? 2 * r.L_out - 1 : r.L_out;
  a.tiles_m = (a.L_res + jg_conv_f16_tile_m() - 1) / jg_conv_f16_tile_m();
  a.out_f16s = hp.out_f16s ? 1 : 0;
  a.act_kind = hp.act_kind;
  a.n_hst = hp.n_hst;
  a.ep = hp.ep;
  a.alpha1 = hp.alpha1; a.alpha2 = hp.alpha2;
  a.dytmask1 = hp.dytmask1; a.dytmask2 = hp.dytmask2;
  a.n_epi_rows = hp.n_epi_rows;
  a.epi = hp.d_epi;
  for (int q = 0; q < hp.n_hst; ++q) a.hst[q] = hp.hst[q];
  if (hp.add_slot >= 0) a.addh = reinterpret_cast<const uint4 *>(m->act[hp.add_slot]);
  if (hp.nmd_slot >= 0) a.nmd_out = m->nmd_part[hp.nmd_slot];
  if (hp.nmd_slot2 >= 0) a.nmd_out2 = m->nmd_part[hp.nmd_slot2];
  a.ep_rt = hp.ep_rt;
  if (hp.d_lut != nullptr) {
    a.lut = hp.d_lut;
    a.lut_vocab = m->vocab;
    a.epi = hp.d_epi_lut;
    a.lut_one_half = op.cout <= 64 ? 1 : 0;
  }
}

// Window-packed tiling when the frames fill their own 256-position tiles badly (e.g. 665 codons); records the partial
// rows (128- / 64-position wave strips) per window that the readers of the conv's NMD taps and fused pool go by
static void conv_f16_tiling(jg_model *m, size_t i, const OpShape &r, int nw, ConvHArgs &a) {
  static const bool no_flat = jg_exp_env("JG_NO_FLAT") != nullptr;
  const jg_op &op = m->ops[i];
  const ConvHPrep &hp = m->hprep[i];
  const int frames = r.in.frames, lo = r.L_out;
  const int strips = hp.cw == 128 ? 2 : 4;               // wave strips per 256-position tile
  int strips_per_win = frames * a.tiles_m * strips;
  const int halo = (a.k - 1) * a.dil;
  const int gap = std::max(a.pad_left, halo - a.pad_left);
  const int fp = lo + gap;
  // a window's pitch: a multiple of the strip height (128) when the conv leaves per-strip partial rows (NMD taps, the
  // fused max pool: a strip must not straddle two windows), else only of 32 - at 83 positions and dilation 8
  // (six frames of 99) 608 instead of 640 positions per window
  const bool strip_rows = hp.nmd_slot >= 0 || hp.nmd_slot2 >= 0 || hp.pool_op >= 0;
  const int wp_unit = strip_rows ? 128 : 32;
  const int wp = (frames * fp + wp_unit - 1) / wp_unit * wp_unit;
  const int64_t flat_tiles = ((int64_t)nw * wp + 255) / 256;
  const int64_t row_tiles = (int64_t)a.rows * a.tiles_m;
  if (!no_flat && a.k == 5 && op.in_buf != JG_BUF_IDS && hp.d_lut == nullptr && a.ostride == 1 && a.L_in == lo &&
      ((op.cout == 128 && !hp.as_k5 && hp.ps_read == 0 && !hp.ps_store) ? jg_conv_f16_has_flat_pattern(hp.ep) : jg_conv_f16_has_narrow_pattern(hp.ep)) &&
      (int64_t)nw * wp < (1 << 24) && flat_tiles * 100 <= row_tiles * 95) {
    a.flat = 1;
    a.flat_p = fp;
    a.flat_wp = wp;
    a.flat_frames = frames;
    a.flat_tiles = (int)flat_tiles;
    a.flat_inv_p = 1.0f / (float)fp;
    a.flat_inv_wp = 1.0f / (float)wp;
    strips_per_win = wp / (256 / strips);
  }
  m->tap_flat = a.flat;
  if (hp.nmd_slot >= 0) m->part_rows[hp.nmd_slot] = strips_per_win;
  if (hp.nmd_slot2 >= 0) m->part_rows[hp.nmd_slot2] = strips_per_win;
  if (hp.pool_op >= 0) m->pool_rows = strips_per_win;
}

// ---- test readback: the template instance of each split-f16 conv launch (JG_MSTAT_TAP_INSTANCE) ----------------------
// Kept per (model, conv op) while a tap is set: the first launch's instance (0: the dispatch has none for it), whether a
// later launch of the same forward ran on another one, and that other one.  Host bookkeeping only, behind one mutex (the
// records of all models share a map; another thread may create, query or destroy its own model meanwhile); an untapped
// forward records nothing and takes no lock.
namespace {
struct ConvInst { bool seen = false; int64_t first = 0, other = 0; };
std::map<std::pair<const jg_model *, int>, ConvInst> conv_inst;
std::mutex conv_inst_mu;
}  // namespace

static void conv_inst_record(const jg_model *m, size_t i, int64_t code) {
  std::lock_guard<std::mutex> lock(conv_inst_mu);
  ConvInst &c = conv_inst[{m, (int)i}];
  if (!c.seen) { c.seen = true; c.first = code; }
  else if (code != (c.first & ~JG_INST_MIXED)) { c.first |= JG_INST_MIXED; c.other = code; }
}

void jg_conv_inst_reset(const jg_model *m) {      // a new forward (or the model goes away): forget the model's records
  std::lock_guard<std::mutex> lock(conv_inst_mu);
  auto it = conv_inst.lower_bound({m, -1});      // (-1: the tapped op's index, below)
  while (it != conv_inst.end() && it->first.first == m) it = conv_inst.erase(it);
}

static void conv_inst_begin(const jg_model *m) {  // a forward with a tap set: fresh records, and which op is tapped
  jg_conv_inst_reset(m);
  std::lock_guard<std::mutex> lock(conv_inst_mu);
  conv_inst[{m, -1}].first = m->tap_op;
}

// op = -1: the op that was tapped in the last forward with a tap (the tap itself is off again by the time tests ask)
int64_t jg_conv_inst_get(const jg_model *m, int op, bool other) {
  std::lock_guard<std::mutex> lock(conv_inst_mu);
  if (op < 0) {
    const auto t = conv_inst.find({m, -1});
    if (t == conv_inst.end()) return 0;
    op = (int)t->second.first;
  }
  const auto it = conv_inst.find({m, op});
  return it == conv_inst.end() ? 0 : other ? it->second.other : it->second.first;
}

static int launch_conv_f16(jg_model *m, size_t i, const OpShape &r, const uint8_t *d_ids, int nw, hipStream_t s) {
  jg_engine *e = m->e;
  const jg_op &op = m->ops[i];
  const ConvHPrep &hp = m->hprep[i];
  ConvHArgs a;
  conv_f16_args(m, i, r, d_ids, nw, a);
  conv_f16_tiling(m, i, r, nw, a);
  if (hp.pool_op >= 0) {       // the fused max pool's partial rows: one per wave strip of the row tiling
    const int64_t need = (int64_t)a.rows * a.tiles_m * (hp.cw == 128 ? 2 : 4) * op.cout;
    if (need > m->pool_part_cap) {
      JG_HIP(hipStreamSynchronize(s));
      if (m->pool_part) (void)hipFree(m->pool_part);
      m->pool_part = nullptr;
      JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->pool_part), (size_t)need * sizeof(float)));
      m->pool_part_cap = need;
      const int prc = poison_fill(e, m->pool_part, need * (int64_t)sizeof(float), s);
      if (prc != JG_OK) return prc;
    }
    a.pool_out = m->pool_part;
  }
  ProfEvent pe;
  int rc = prof_begin(e, s, hp.d_lut != nullptr ? JG_PROF_TABLE : JG_PROF_MFMA_F16X3, conv_flops(op, r, nw), &pe);
  if (rc != JG_OK) return rc;
  // with a tap set, the launcher that runs names its instance; a dispatch without one fails and is recorded as 0, a call
  // that launches nothing (an empty batch) returns JG_OK without a code and is not recorded
  const bool tapped = m->tap_op >= 0;
  for (int hf = 0; hf < hp.n_half && rc == JG_OK; ++hf) {      // wider than 128 channels: one launch per 128
    if (hf > 0) {
      a.ch0 = hf * 128;
      a.wh = hp.ps_read == 1 ? hp.d_wh_ps[r.in.L & 1] + (int64_t)hf * hp.ps_half_items : hp.d_wh + (int64_t)hf * hp.wh_half_items;
      a.epi = hp.d_epi + (int64_t)hf * hp.n_epi_rows * 2 * 128;
    }
    int64_t code = 0;
    rc = jg_launch_conv_f16(e, a, s, tapped ? &code : nullptr);
    if (tapped && (code != 0 || rc != JG_OK)) conv_inst_record(m, i, code);
  }
  return prof_end(e, s, &pe, rc);
}

static int f32_tiles(int L) { return (L + jg_conv_tile_m(L) - 1) / jg_conv_tile_m(L); }   // tiles per row of the f32 kernels

static int launch_conv_f32(jg_model *m, size_t i, const OpShape &r, const uint8_t *d_ids, int nw, hipStream_t s) {
  jg_engine *e = m->e;
  const jg_op &op = m->ops[i];
  const int lo = r.L_out;
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = op.in_buf == JG_BUF_IDS ? nullptr : m->act[op.in_buf];
  a.ids = op.in_buf == JG_BUF_IDS ? d_ids : nullptr;
  a.emb = op.in_buf == JG_BUF_IDS ? m->d_w + op.b_off : nullptr;
  a.mask_from_ids = op.in_mask == JG_BUF_IDS;
  a.mask_in = op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr;
  a.mask_out = op.out_mask >= 0 ? m->msk[op.out_mask] : nullptr;
  a.w = m->d_w + op.w_off;
  a.w8 = m->hprep[i].d_w8;
  a.y = m->act[op.out_buf];
  a.rows = nw * r.in.frames;
  a.L_in = r.in.L; a.L_out = lo;
  a.cin = op.cin; a.cin_pad = (op.cin + 7) / 8 * 8;
  a.cout = op.cout; a.cout_pad = (op.cout + 31) / 32 * 32;
  a.k = op.k; a.stride = op.stride; a.dil = op.dilation; a.pad_left = r.pad_left;
  const int tm = jg_conv_tile_m_for(lo, op.k, op.cin, op.stride, op.dilation);
  a.tiles_m = (lo + tm - 1) / tm;
  for (int q = 0; q < op.n_stages; ++q)
    if (op.stages[q].kind == JG_ST_NMD) m->part_rows[op.stages[q].arg] = r.in.frames * a.tiles_m;
  resolve_stages(m, op, a.st, &a.n_stages);
  ProfEvent pe;
  int rc = prof_begin(e, s, JG_PROF_MFMA_F32, conv_flops(op, r, nw), &pe);
  if (rc != JG_OK) return rc;
  return prof_end(e, s, &pe, jg_launch_conv(e, a, s));
}

static int launch_eltwise(jg_model *m, size_t i, const OpShape &r, int nw, hipStream_t s) {
  const jg_op &op = m->ops[i];
  const Shape &in = r.in;
  EltArgs a;
  memset(&a, 0, sizeof(a));
  a.x = m->act[op.in_buf];
  a.y = m->act[op.out_buf];
  a.mask = op.out_mask >= 0 ? m->msk[op.out_mask] : nullptr;
  a.n_pos = (int64_t)nw * in.frames * in.L;
  a.c = in.C;
  for (int q = 0; q < op.n_stages; ++q)
    if (op.stages[q].kind == JG_ST_NMD) m->part_rows[op.stages[q].arg] = in.frames * f32_tiles(in.L);
  resolve_stages(m, op, a.st, &a.n_stages);
  if (a.n_stages > 0 && a.st[0].kind == JG_ST_LN) return jg_launch_layernorm(a, nw * in.frames, in.L, f32_tiles(in.L), s);
  return jg_launch_eltwise(a, s);
}

// the fields the row mixers' argument structs share (frame attention counts windows and has no mask)
static void mixer_rows(JgFrameAttnArgs &a, const uint8_t *, int nw, int) { a.n_win = nw; }
template <typename Args>
static void mixer_rows(Args &a, const uint8_t *mask, int nw, int frames) {
  a.mask = mask;
  a.rows = nw * frames;
}
template <typename Args>
static void mixer_args(const jg_model *m, const jg_op &op, const OpShape &r, int nw, int tile, Args &a) {
  memset(&a, 0, sizeof(a));
  a.x = m->act[op.in_buf];
  a.y = m->act[op.out_buf];
  a.w = m->d_w + op.w_off;
  mixer_rows(a, op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr, nw, r.in.frames);
  a.L = r.in.L; a.tiles = (r.in.L + tile - 1) / tile;
  a.C = op.cin;
  a.eps = op.f0;
  resolve_stages(m, op, a.st, &a.n_stages);
}

// A row mixer: f32 rows from in_buf to out_buf, validity from the op's mask slot (which it leaves as it is).  Length attention
// and hyena have no profiling class (scripts/lengthattn_perf.py and scripts/hyena_perf.py time them with events around whole
// programs); hyena's p_0 .. p_order go through the model's projection scratch (jg_ensure_workspace sized it from the shape walk)
static int launch_mixer(jg_model *m, size_t i, const OpShape &r, int nw, hipStream_t s) {
  jg_engine *e = m->e;
  const jg_op &op = m->ops[i];
  const int prof = jg_mixer_kind(op.kind)->prof;
  const int64_t scratch = (int64_t)nw * r.scratch * (int64_t)sizeof(float);
  JG_REQUIRE(scratch <= m->hy_cap, JG_ERR_INVALID, "op %zu: hyena scratch of %lld bytes, %lld needed", i, (long long)m->hy_cap, (long long)scratch);
  ProfEvent pe;
  int rc = prof >= 0 ? prof_begin(e, s, prof, jg_mixer_flops(m, i, r, nw), &pe) : JG_OK;
  if (rc != JG_OK) return rc;
  switch (op.kind) {
    case JG_OP_FRAMEATTN: {
      JgFrameAttnArgs a;
      mixer_args(m, op, r, nw, 16, a);
      a.H = op.k; a.D = op.cin / op.k; a.F = op.arg;
      rc = jg_launch_frameattn(e, a, s);
    } break;
    case JG_OP_LOCALATTN: {
      JgLocalAttnArgs a;
      mixer_args(m, op, r, nw, JG_LOCALATTN_TILE, a);
      a.H = op.k; a.D = op.cin / op.k; a.F = op.arg;
      a.half = op.stride;
      rc = jg_launch_localattn(e, a, s);
    } break;
    case JG_OP_LENGTHATTN: {
      JgLengthAttnArgs a;
      mixer_args(m, op, r, nw, JG_LENGTHATTN_TILE, a);
      a.H = op.k; a.D = op.cin / op.k; a.F = op.arg;
      rc = jg_launch_lengthattn(e, a, s);
    } break;
    case JG_OP_BILSTM: {
      JgBilstmArgs a;
      mixer_args(m, op, r, nw, JG_BILSTM_STEPS, a);
      a.U = op.k;
      if (op.arg & JG_BILSTM_IGNORE_MASK) a.mask = nullptr;
      rc = jg_launch_bilstm(e, a, s);
    } break;
    case JG_OP_MSCONV: {
      JgMsconvArgs a;
      mixer_args(m, op, r, nw, JG_MSCONV_TILE, a);
      a.cout = op.cout; a.n_branches = op.k; a.merge = op.arg;
      a.halo_l = m->hprep[i].ms_halo_l; a.halo_r = m->hprep[i].ms_halo_r;
      rc = jg_launch_msconv(e, a, s);
    } break;
    default: {      // JG_OP_HYENA
      JgHyenaArgs a;
      mixer_args(m, op, r, nw, JG_HYENA_TILE, a);
      a.scratch = m->hy_scratch;
      a.order = op.k; a.table_rows = op.stride;
      a.out_proj = (op.arg & JG_HYENA_OUT_PROJ) != 0; a.normalize = (op.arg & JG_HYENA_NORMALIZE) != 0;
      rc = jg_launch_hyena(e, a, s);
    } break;
  }
  return prof >= 0 ? prof_end(e, s, &pe, rc) : rc;
}

static int launch_nmd_final(jg_model *m, size_t i, const OpShape &r, int nw, hipStream_t s) {
  // op.arg = partial slot, in_mask = mask the tap used, cout = channels,
  // in_buf = activation slot whose shape gives the position count
  const jg_op &op = m->ops[i];
  const Shape &in = r.in;
  // partial rows per window as the tap that filled the slot laid them out (a conv records it; an element-wise
  // LayerNorm tap uses the f32 tiling of the slot)
  const int rows_per_win = m->part_rows[op.arg] > 0 ? m->part_rows[op.arg] : in.frames * f32_tiles(in.L);
  const uint8_t *mk = op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr;
  return jg_launch_nmd_final(m->nmd_part[op.arg], rows_per_win, mk, in.frames * in.L, m->d_w + op.b_off, op.f0, nw, op.cout,
                             m->vec[op.out_vec], m->vec_w[op.out_vec], op.vec_off, s);
}

// the op's own kernel
static int launch_ordinary(jg_model *m, size_t i, const OpShape &r, const uint8_t *d_ids, int nw, hipStream_t s) {
  const jg_op &op = m->ops[i];
  const Shape &in = r.in;
  float *const out_vec = op.out_vec >= 0 ? m->vec[op.out_vec] : nullptr;
  const int out_ld = op.out_vec >= 0 ? m->vec_w[op.out_vec] : 0;
  switch (op.kind) {
    case JG_OP_EMBED:
      return jg_launch_embed_pos(d_ids, m->id_bytes, (int64_t)nw * m->id_frames * r.out.L, r.out.L, m->d_w + op.b_off, m->vocab, op.cout,
                                 op.w_off >= 0 ? m->d_w + op.w_off : nullptr, m->act[op.out_buf], m->msk[op.out_mask], s);
    case JG_OP_MASK:
      return jg_launch_mask(op.in_mask == JG_BUF_IDS ? d_ids : m->msk[op.in_mask], nw * m->id_frames, r.m_in, r.L_out, op.k, op.stride,
                            op.dilation, r.pad_left, op.mask_mode, m->msk[op.out_mask], s);
    case JG_OP_MSMASK:
      return jg_launch_msmask(m->msk[op.in_mask], nw * m->id_frames, r.m_in, m->d_w + op.w_off, op.k, m->msk[op.out_mask], s);
    case JG_OP_ELTWISE: return launch_eltwise(m, i, r, nw, s);
    case JG_OP_MAXPOOL1D:
      if (m->precision == 1 && m->hprep[i].pool_f16s)
        return jg_launch_maxpool1d_f16s(reinterpret_cast<const uint4 *>(m->act[op.in_buf]), nw * in.frames, in.L, r.L_out, in.C,
                                        reinterpret_cast<uint4 *>(m->act[op.out_buf]), s);
      return jg_launch_maxpool1d(m->act[op.in_buf], nullptr, nw * in.frames, in.L, r.L_out, in.C, m->act[op.out_buf], nullptr, s);
    case JG_OP_FRAMESUM:
      return jg_launch_framesum(m->act[op.in_buf], nw, in.frames, (int64_t)in.L * in.C, m->act[op.out_buf], s);
    case JG_OP_POOL:
      return jg_launch_pool(m->act[op.in_buf], op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr, nw, in.frames * in.L, in.C, op.arg,
                            out_vec + op.vec_off, out_ld, s);
    case JG_OP_POOLVEC: {
      JgPoolVecArgs a;
      memset(&a, 0, sizeof(a));
      a.x = m->act[op.in_buf]; a.mask = op.in_mask >= 0 ? m->msk[op.in_mask] : nullptr;
      a.out = out_vec + op.vec_off; a.out_ld = out_ld;
      a.n_win = nw; a.frames = in.frames; a.L = in.L; a.c = in.C;
      a.kind = op.arg; a.merge = op.k; a.scale = op.f0;
      return jg_launch_poolvec(a, s);
    }
    case JG_OP_DENSE:
      return jg_launch_dense(m->vec[op.in_vec], m->vec_w[op.in_vec], m->d_w + op.w_off, op.b_off >= 0 ? m->d_w + op.b_off : nullptr,
                             nw, op.cin, op.cout, op.arg, out_vec + op.vec_off, out_ld, s);
    case JG_OP_NMD_FINAL: return launch_nmd_final(m, i, r, nw, s);
    case JG_OP_OODSIG:
      // in_vec = logits (cin classes), op.k = nmd vector slot (width op.stride), arg = order
      return jg_launch_oodsig(m->vec[op.in_vec], m->vec_w[op.in_vec], op.cin, m->vec[op.k], m->vec_w[op.k], op.stride, nw,
                              (unsigned)op.arg, op.f0, out_vec, out_ld, op.vec_off, s);
    case JG_OP_VECMAX:
      return jg_launch_vecmax(m->vec[op.in_vec], m->vec_w[op.in_vec], op.k, op.cout, nw, out_vec, out_ld, op.vec_off, s);
    case JG_OP_STRANDS:      // the strands' rows are merged into the window's behind the program (jg_forward_chunks)
      return JG_OK;
    default:
      jg_set_error("op %zu: kind %d not implemented", i, op.kind);
      return JG_ERR_UNSUPPORTED;
  }
}

// Run the op program over `nw` windows whose ids (nw, 6, l) are on the device (a two-strand model: nw = strand rows,
// ids (nw, 1, l)).  Per op: the layout conversions in front of it, the launcher of its placement, the tap.
static int run_chunk(jg_model *m, const std::vector<OpShape> &shp, const uint8_t *d_ids, int nw, int l, hipStream_t s) {
  const PlaceCtx pc = jg_place_ctx(m, &shp, l);
  int rc = JG_OK;
  if (pc.small && (rc = launch_small_net(m, shp[small_conv0(m)], d_ids, nw, s)) != JG_OK) return rc;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    const OpShape &r = shp[i];
    const Place pl = jg_place_op(m, i, pc);
    char why[256];
    if ((int)i == m->tap_op && jg_tap_refusal(m, i, pc, l, why, sizeof(why)) != nullptr) {
      jg_set_error("tap: %s", why);
      return JG_ERR_UNSUPPORTED;
    }
    // (ops inside the small-window kernel read no tensor: nothing is converted for them)
    if (pc.prec == 1 && pl != PL_SMALL_SKIP && pl != PL_SMALL_NMD && (rc = convert_layouts(m, i, r, nw, s)) != JG_OK) return rc;
    switch (pl) {
      case PL_SMALL_SKIP: case PL_TAB_POOL: case PL_RB_CONV1: break;          // computed by another op's launch
      case PL_SMALL_NMD: rc = launch_small_nmd(m, i, nw, s); break;
      case PL_SMALL_POOL:
        rc = jg_launch_small_pool_final(m->small->d_part, 6, m->small->n_slots, 0, nw, m->small->pool_kind, nullptr, 0.f,
                                        m->vec[op.out_vec] + op.vec_off, m->vec_w[op.out_vec], s);
        break;
      case PL_TAB_CONV: rc = launch_tab_net(m, i, r, d_ids, nw, s); break;
      case PL_RB32: case PL_RB64: rc = launch_resblock(m, i, r, nw, s, pl == PL_RB64); break;
      case PL_CONV_F16: rc = launch_conv_f16(m, i, r, d_ids, nw, s); break;
      case PL_CONV_F32: rc = launch_conv_f32(m, i, r, d_ids, nw, s); break;
      case PL_POOL_FUSED:
        rc = jg_launch_pool_final(m->pool_part, m->pool_rows, nw, r.in.C, m->vec[op.out_vec] + op.vec_off, m->vec_w[op.out_vec], s);
        break;
      case PL_MIXER: rc = launch_mixer(m, i, r, nw, s); break;
      case PL_ORDINARY: rc = launch_ordinary(m, i, r, d_ids, nw, s); break;
    }
    if (rc != JG_OK) return rc;
    if ((int)i == m->tap_op && (rc = jg_tap_copy(m, i, r, pc, nw, s)) != JG_OK) return rc;
  }
  return JG_OK;
}

static int copy_out(jg_model *m, int slot, int width, float *dst, int64_t row0, int nw, int out_loc,
                    hipStream_t s) {
  if (dst == nullptr || width <= 0) return JG_OK;
  JG_REQUIRE(m->vec[slot] != nullptr, JG_ERR_INVALID,
             "output requested but the model does not produce vector slot %d", slot);
  const hipMemcpyKind kind = out_loc == JG_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const float *src = m->vec[slot];
  size_t src_ld = (size_t)m->vec_w[slot];
  if (m->strands > 1) {
    // branched model: the vector slot holds one row per strand; the window's row is their merge (the prediction by the
    // classifier's merge layer, every other output by Average - builder.py:776-791)
    const int64_t had = m->merged_cap[slot];
    int rc = grow(&m->merged[slot], &m->merged_cap[slot], (int64_t)nw * width * (int64_t)sizeof(float));
    if (rc != JG_OK || (m->merged_cap[slot] != had && (rc = poison_fill(m->e, m->merged[slot], m->merged_cap[slot], s)) != JG_OK)) return rc;
    const int kind = slot == 2 ? m->merge_kind : JG_MERGE_AVERAGE;
    // (`width` is the OUTPUT's: a concatenated prediction is `strands` head vectors wide)
    const int mrc = jg_launch_strand_merge(src, (int)src_ld, nw, m->strands, kind == JG_MERGE_CONCAT ? width / m->strands : width, kind,
                                           m->merged[slot], s);
    if (mrc != JG_OK) return mrc;
    src = m->merged[slot];
    src_ld = (size_t)width;
  }
  JG_HIP(hipMemcpy2DAsync(dst + row0 * width, (size_t)width * sizeof(float), src, src_ld * sizeof(float),
                          (size_t)width * sizeof(float), (size_t)nw, kind, s));
  return JG_OK;
}

// windows per launch group: amortises launch + pipeline fill.  2 048 windows of 498 codons per frame (+0.7 % over
// 1 024; 3.1 GB per activation slot), proportionally more for shorter frames (same positions: +6 % at 500 bp),
// and the 32-bit DMA offset cap below for longer ones
int jg_effective_chunk(const jg_model *m, int chunk, int l, int64_t n_win) {
  if (chunk <= 0) chunk = (int)std::min<int64_t>(65536, std::max<int64_t>(1024, (int64_t)2048 * 498 / std::max(l, 1) / 256 * 256));
  // split-f16 DMA offsets are 32-bit: keep one activation tensor (6 frames x l x 512 B) < 3.5 GB
  if (m->precision == 1) {
    const int64_t cap = (int64_t)(3.5e9 / (6.0 * l * 512.0));
    if (chunk > cap) chunk = (int)std::max<int64_t>(cap, 1);
  }
  if (chunk > n_win) chunk = (int)std::max<int64_t>(n_win, 1);
  return chunk;
}

// enqueue only: the chunk loop of one id tensor (workspace already sized for `chunk`); no range-guard readback
int jg_forward_chunks(jg_model *m, const std::vector<OpShape> &shp, const uint8_t *d_ids, int64_t n_win, int l, float *prediction,
                      float *reliability, float *embedding, float *nmd, int out_loc, int chunk, hipStream_t s) {
  const int w_pred = jg_model_vec_width(m, 0), w_rel = jg_model_vec_width(m, 1);
  const int w_emb = jg_model_vec_width(m, 2), w_nmd = jg_model_vec_width(m, 3);
  for (int64_t w0 = 0; w0 < n_win; w0 += chunk) {
    const int nw = (int)std::min<int64_t>(chunk, n_win - w0);
    m->tap_row0 = w0 * m->strands;
    int rc = poison_workspace(m, s);
    if (rc != JG_OK) return rc;
    rc = run_chunk(m, shp, d_ids + w0 * m->strands * m->id_frames * (int64_t)l * m->id_bytes, nw * m->strands, l, s);
    if (rc != JG_OK) return rc;
    if ((rc = copy_out(m, 2, w_pred, prediction, w0, nw, out_loc, s)) != JG_OK) return rc;
    if ((rc = copy_out(m, 3, w_rel, reliability, w0, nw, out_loc, s)) != JG_OK) return rc;
    if ((rc = copy_out(m, 0, w_emb, embedding, w0, nw, out_loc, s)) != JG_OK) return rc;
    if ((rc = copy_out(m, 1, w_nmd, nmd, w0, nw, out_loc, s)) != JG_OK) return rc;
  }
  return JG_OK;
}

int jg_forward_device_ids(jg_model *m, const uint8_t *d_ids, int64_t n_win, int l, float *prediction, float *reliability,
                          float *embedding, float *nmd, int out_loc, int chunk, hipStream_t s) {
  chunk = jg_effective_chunk(m, chunk, l, n_win);
  JG_REQUIRE((int64_t)chunk * 6 <= 0x7fffffff / 8, JG_ERR_INVALID, "chunk too large");
  std::vector<OpShape> shp;                // one shape walk per call: the workspace and every chunk read it
  int rc = jg_shape_walk(m, l, shp);
  if (rc != JG_OK || (rc = jg_ensure_workspace(m, (int64_t)chunk * m->strands, l, shp)) != JG_OK) return rc;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = jg_forward_chunks(m, shp, d_ids, n_win, l, prediction, reliability, embedding, nmd, out_loc, chunk, s)) != JG_OK)
      return rc;
    if (m->precision != 1) break;
    // split-f16 range guard: an activation beyond the f16 range poisons the fast path;
    // fall back to the exact-f32 kernels for this and every later call of the model.
    int flag = 0;
    JG_HIP(hipMemcpyAsync(&flag, m->d_overflow, sizeof(int), hipMemcpyDeviceToHost, s));
    JG_HIP(hipStreamSynchronize(s));
    if (flag == 0) break;
    JG_HIP(hipMemsetAsync(m->d_overflow, 0, sizeof(int), s));
    m->precision = 0;
    m->f16_reason = "an activation left the f16 range at run time";
  }
  return JG_OK;
}

extern "C" int jg_forward(jg_model *m, const uint8_t *ids, int ids_loc, int64_t n_win, int32_t l,
                          float *prediction, float *reliability, float *embedding, float *nmd,
                          int out_loc, int32_t chunk, void *stream) {
  JG_REQUIRE(m != nullptr && ids != nullptr && n_win >= 0 && l > 0, JG_ERR_INVALID,
             "jg_forward: bad arguments");
  if (n_win == 0) return JG_OK;
  jg_engine *e = m->e;
  JG_HIP(hipSetDevice(e->dev));
  hipStream_t s = pick_stream(e, stream);
  m->tap_variant = 0;
  if (m->tap_op >= 0) conv_inst_begin(m);
  const uint8_t *d_ids = ids;
  if (ids_loc == JG_PTR_HOST) {
    const int64_t bytes = n_win * m->strands * m->id_frames * (int64_t)l * m->id_bytes;
    int rc = grow(&m->d_ids, &m->d_ids_cap, bytes);
    if (rc != JG_OK) return rc;
    JG_HIP(hipMemcpyAsync(m->d_ids, ids, (size_t)bytes, hipMemcpyHostToDevice, s));
    d_ids = m->d_ids;
  }
  int rc = jg_forward_device_ids(m, d_ids, n_win, l, prediction, reliability, embedding, nmd, out_loc, chunk, s);
  if (rc != JG_OK) return rc;
  if (out_loc == JG_PTR_HOST || ids_loc == JG_PTR_HOST) JG_HIP(hipStreamSynchronize(s));
  return JG_OK;
}
