// C-ABI of libjaeger_hip.so, model part: program validation, the shape walk, model create / destroy, describe() and
// the statistics, the workspace, and the test readback (taps).  Host logic only.
#include <stdio.h>

#include "jg_host.h"

static void conv_geometry(int L_in, int k, int stride, int dil, int padding, int *L_out, int *pad_left) {
  if (padding == JG_PAD_SAME) {
    // TF 'SAME': L_out = ceil(L/s); pad_left = pad_total // 2
    const int lo = (L_in + stride - 1) / stride;
    int total = (lo - 1) * stride + (k - 1) * dil + 1 - L_in;
    if (total < 0) total = 0;
    *L_out = lo;
    *pad_left = total / 2;
  } else {
    const int span = dil * (k - 1) + 1;
    *L_out = L_in >= span ? (L_in - span) / stride + 1 : 0;
    *pad_left = 0;
  }
}

// ---- row mixers: the questions with kind-specific arithmetic, one switch each (the rest is jg_mixer_kinds) ------------
// op fields: cin = cout = channels, f0 = the layer norms' epsilon, w_off = the packed weights; the attention ops: k = heads,
// arg = feed-forward width (frame attention: 0 = no feed-forward half), local attention: stride = half-window; hyena:
// k = order, arg = flags, stride = rows of the filter table; bilstm: cin = C, cout = 2 k, k = units, arg = flags, no epsilon;
// multi-scale conv: cin, cout, k = branches, arg = merge kind, no epsilon - the rest in the descriptor at w_off (msconv_desc)
static bool mixer_supports(const jg_op &op, char *why, size_t cap) {      // sizes the kernel covers (why: the reason when not)
  switch (op.kind) {
    case JG_OP_MSCONV: return jg_msconv_supports(op.cin, op.k, op.cout, op.arg, why, cap);
    case JG_OP_FRAMEATTN: return jg_frameattn_supports(op.cin, op.k, op.arg, why, cap);
    case JG_OP_LOCALATTN: return jg_localattn_supports(op.cin, op.k, op.arg, op.stride, why, cap);
    case JG_OP_LENGTHATTN: return jg_lengthattn_supports(op.cin, op.k, op.arg, why, cap);
    case JG_OP_HYENA: return jg_hyena_supports(op.cin, op.k, op.stride, why, cap);
    default: return jg_bilstm_supports(op.cin, op.k, op.cout, why, cap);
  }
}

// the descriptor of a multi-scale conv op or of its mask op out of the host blob jg_model_create was given, validated
static int msconv_desc(const jg_model *m, size_t i, const float *weights, JgMsconvDesc *d) {
  const jg_op &op = m->ops[i];
  JG_REQUIRE(op.w_off >= 0 && op.w_off < m->n_w, JG_ERR_INVALID, "op %zu: multi-scale conv descriptor outside the weight blob", i);
  char why[200];
  const int rc = jg_msconv_read_desc(weights + op.w_off, m->n_w - op.w_off, op.cin, op.k, op.cout, op.arg, d, why, sizeof(why));
  if (rc != JG_OK) jg_set_error("op %zu: multi-scale conv with %s", i, why);
  return rc;
}

static int64_t mixer_blob_floats(const jg_op &op) {      // (multi-scale conv: the descriptor; msconv_desc checks what it names)
  switch (op.kind) {
    case JG_OP_MSCONV: return JG_MSCONV_DESC_FLOATS;
    case JG_OP_FRAMEATTN: return jg_frameattn_blob_floats(op.cin, op.arg);
    case JG_OP_LOCALATTN: return jg_localattn_blob_floats(op.cin, op.arg);
    case JG_OP_LENGTHATTN: return jg_lengthattn_blob_floats(op.cin, op.arg);
    case JG_OP_HYENA: return jg_hyena_blob_floats(op.cin, op.k, op.stride, op.arg);
    default: return jg_bilstm_blob_floats(op.cin, op.k);
  }
}

static int64_t mixer_lds_bytes(const jg_op &op) {      // where the size depends on the op (0: a fixed size that always fits)
  switch (op.kind) {
    case JG_OP_LOCALATTN: return jg_localattn_lds_bytes(op.cin, op.cin / op.k, op.stride);
    case JG_OP_LENGTHATTN: return jg_lengthattn_lds_bytes(op.cin, op.k);
    case JG_OP_BILSTM: return jg_bilstm_lds_bytes(op.cin, op.k);
    default: return 0;
  }
}

static int64_t mixer_row_scratch(const jg_op &op, int L) {      // floats of scratch one row of L positions needs
  return op.kind == JG_OP_HYENA ? jg_hyena_row_scratch(op.cin, op.k, L) : 0;
}

double jg_mixer_flops(const jg_model *m, size_t i, const OpShape &r, int nw) {
  const jg_op &op = m->ops[i];
  const int C = op.cin, L = r.in.L;
  const double rows = (double)(nw * r.in.frames);
  switch (op.kind) {
    case JG_OP_FRAMEATTN:      // the four dense products
      return 2.0 * (4.0 * C * C + 2.0 * C * op.arg) * rows * L;
    case JG_OP_LOCALATTN: {
      // q, the projection and the feed-forward half per position; k and v per position and per halo position of its tile
      const int hb = (op.stride + 15) / 16;
      const double kv_share = (double)(JG_LOCALATTN_TILE + 32 * hb) / JG_LOCALATTN_TILE;
      return 2.0 * ((2.0 + 2.0 * kv_share) * C * C + 2.0 * C * op.arg) * rows * L;
    }
    case JG_OP_LENGTHATTN: {   // dense products (k and v once per query tile) plus 4 L^2 C of scores and context
      const double tiles = (L + JG_LENGTHATTN_TILE - 1) / JG_LENGTHATTN_TILE;
      return (2.0 * (2.0 * C * C + 2.0 * C * op.arg) * L + 2.0 * (2.0 * C * C) * L * tiles + 4.0 * (double)L * L * C) * rows;
    }
    case JG_OP_HYENA: {        // the projections and 2 x order x C x L (L + 1) / 2 of the convolutions
      const double dense = 2.0 * (op.k + 1 + ((op.arg & JG_HYENA_OUT_PROJ) ? 1 : 0)) * C * C * (double)L;
      return (dense + 2.0 * op.k * C * ((double)L * (L + 1) / 2)) * rows;
    }
    case JG_OP_MSCONV:         // per position and branch taps x cin x filters multiply-adds (the padded columns are not counted)
      return rows * L * 2.0 * C * (double)m->hprep[i].ms_macs;
    default:                   // bilstm: x W and h R of the two directions (the element-wise work is not counted)
      return rows * L * 2.0 * (2.0 * C * 4.0 * op.k + 2.0 * op.k * 4.0 * op.k);
  }
}

static int mixer_describe(const jg_op &op, size_t i, char *line, size_t cap) {      // without the conversion note and the newline
  switch (op.kind) {
    case JG_OP_FRAMEATTN:
      return snprintf(line, cap, "op %zu: frame attention c=%d heads=%d key_dim=%d ff=%d -> one launch, exact-f32 matrix cores, f32 rows",
                      i, op.cin, op.k, op.cin / op.k, op.arg);
    case JG_OP_LOCALATTN:
      return snprintf(line, cap, "op %zu: local attention c=%d heads=%d key_dim=%d ff=%d half_window=%d %s -> one launch, exact-f32 matrix cores, f32 rows",
                      i, op.cin, op.k, op.cin / op.k, op.arg, op.stride, op.in_mask >= 0 ? "masked keys" : "no mask");
    case JG_OP_LENGTHATTN:
      return snprintf(line, cap, "op %zu: length attention c=%d heads=%d key_dim=%d ff=%d %s -> one launch, exact-f32 matrix cores (dense), vector ALUs (scores, context), f32 rows",
                      i, op.cin, op.k, op.cin / op.k, op.arg, op.in_mask >= 0 ? "masked queries and keys" : "no mask");
    case JG_OP_MSCONV:
      return snprintf(line, cap, "op %zu: multi-scale conv cin=%d branches=%d merge=%s cout=%d %s -> one launch, %d positions a workgroup, the input tile read once, exact-f32 matrix cores, f32 rows (frames, L, %d)",
                      i, op.cin, op.k, op.arg == JG_MSCONV_ADD ? "add" : "concat", op.cout, op.in_mask >= 0 ? "masked input" : "no mask", JG_MSCONV_TILE, op.cout);
    case JG_OP_BILSTM:
      return snprintf(line, cap, "op %zu: bilstm c=%d units=%d %s -> one launch, %d rows x one direction a workgroup, exact-f32 matrix cores, f32 rows (frames, L, %d)",
                      i, op.cin, op.k, (op.arg & JG_BILSTM_IGNORE_MASK) ? "mask ignored" : op.in_mask >= 0 ? "masked steps carried" : "no mask", JG_BILSTM_ROWS, op.cout);
    default:
      return snprintf(line, cap, "op %zu: hyena c=%d order=%d table_rows=%d%s%s %s -> %d launches: projections on the exact-f32 matrix cores, causal convolutions on the vector ALUs, f32 rows",
                      i, op.cin, op.k, op.stride, (op.arg & JG_HYENA_OUT_PROJ) ? " output_projection" : "", (op.arg & JG_HYENA_NORMALIZE) ? " filter_normalize" : "",
                      op.in_mask >= 0 ? "masked" : "no mask", 2 + op.k);
  }
}

static int validate_mixer(const jg_model *m, size_t i, const float *weights) {
  const jg_op &op = m->ops[i];
  const MixerKind &mk = *jg_mixer_kind(op.kind);
  JG_REQUIRE(op.in_buf >= 0 && op.out_buf >= 0 && (!mk.same_width || (op.cin == op.cout && op.f0 > 0.f)) && (!mk.dilation_1 || op.dilation == 1),
             JG_ERR_INVALID, "op %zu: a %s op reads and writes an activation slot%s", i, mk.noun, mk.same_width ? " of cin = cout channels" : "");
  JG_REQUIRE(mk.in_place || op.in_buf != op.out_buf, JG_ERR_INVALID,
             "op %zu: a %s op cannot run in place (its workgroups read rows that others write)", i, mk.noun);
  const bool mask_slot = op.in_mask >= 0 || op.in_mask == JG_BUF_NONE;
  switch (mk.mask) {
    case MM_NONE:
      JG_REQUIRE(op.out_mask == JG_BUF_NONE, JG_ERR_INVALID, "op %zu: a %s op leaves no mask (out_mask = none)", i, mk.noun);
      break;
    case MM_KEEP:
      JG_REQUIRE(mask_slot && op.out_mask == op.in_mask, JG_ERR_INVALID,
                 "op %zu: a %s op keeps its mask (out_mask = in_mask, a mask slot or none)", i, mk.noun);
      break;
    case MM_KEEP_OR_DROP:
      JG_REQUIRE(mask_slot && (op.out_mask == op.in_mask || op.out_mask == JG_BUF_NONE), JG_ERR_INVALID,
                 "op %zu: a %s op keeps its mask or drops it (out_mask = in_mask or none)", i, mk.noun);
      break;
    case MM_OWN:
      JG_REQUIRE(mask_slot && (op.out_mask >= 0 || op.out_mask == JG_BUF_NONE), JG_ERR_INVALID,
                 "op %zu: a %s op reads a mask slot or none and names the mask slot of its output or none", i, mk.noun);
      break;
  }
  if (op.kind == JG_OP_HYENA)
    JG_REQUIRE((op.arg & ~(JG_HYENA_OUT_PROJ | JG_HYENA_NORMALIZE)) == 0, JG_ERR_INVALID, "op %zu: hyena flags %d", i, op.arg);
  if (op.kind == JG_OP_BILSTM) {
    JG_REQUIRE((op.arg & ~JG_BILSTM_IGNORE_MASK) == 0, JG_ERR_INVALID, "op %zu: bilstm flags %d", i, op.arg);
    JG_REQUIRE(op.out_mask == ((op.arg & JG_BILSTM_IGNORE_MASK) ? JG_BUF_NONE : op.in_mask), JG_ERR_INVALID,
               "op %zu: a bilstm op that ignores the mask leaves none, and one that does not keeps it (out_mask against arg)", i);
  }
  char why[160];
  JG_REQUIRE(mixer_supports(op, why, sizeof(why)), JG_ERR_UNSUPPORTED, "op %zu: %s with %s", i, mk.noun, why);
  JG_REQUIRE(mixer_lds_bytes(op) <= 160 * 1024, JG_ERR_UNSUPPORTED, "op %zu: %s needs %lld bytes of LDS", i, mk.noun, (long long)mixer_lds_bytes(op));
  JG_REQUIRE(m->ops.back().kind != JG_OP_STRANDS, JG_ERR_UNSUPPORTED,
             "op %zu: %s needs the frame rows of a translated window (not a strand program)", i, mk.noun);
  JG_REQUIRE(op.w_off >= 0 && op.w_off + mixer_blob_floats(op) <= m->n_w, JG_ERR_INVALID,
             "op %zu: %s weights outside the weight blob", i, mk.noun);
  if (op.kind == JG_OP_MSCONV) {
    JgMsconvDesc d;
    const int rc = msconv_desc(m, i, weights, &d);
    if (rc != JG_OK) return rc;
    const int64_t lds = jg_msconv_lds_bytes(op.cin, op.cout, d.halo_l, d.halo_r);
    JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "op %zu: %s needs %lld bytes of LDS", i, mk.noun, (long long)lds);
  }
  for (int s = 0; s < op.n_stages; ++s) {
    const int kd = op.stages[s].kind;
    JG_REQUIRE(kd == JG_ST_BIAS || kd == JG_ST_BN || kd == JG_ST_ACT || (kd == JG_ST_DYT && op.stages[s].arg == 0), JG_ERR_UNSUPPORTED,
               "op %zu stage %d: only bias / batch norm / unmasked DyT / activation stages fuse behind %s (kind %d)", i, s, mk.noun, kd);
  }
  return JG_OK;
}

// a pool-and-merge op: arg = the pool, k = the merge, f0 = the scale, cout channels of in_buf into out_vec at vec_off
static int validate_poolvec(const jg_model *m, size_t i) {
  const jg_op &op = m->ops[i];
  JG_REQUIRE(op.in_buf >= 0 && op.out_vec >= 0 && (op.in_mask >= 0 || op.in_mask == JG_BUF_NONE), JG_ERR_INVALID,
             "op %zu: a pool-and-merge op reads an activation slot under a mask slot or none and writes a vector slot", i);
  char why[200];
  JG_REQUIRE(jg_poolvec_supports(op.arg, op.k, op.cout, op.vec_off, why, sizeof(why)), JG_ERR_UNSUPPORTED,
             "op %zu: pool-and-merge with %s", i, why);
  JG_REQUIRE(m->ops.back().kind != JG_OP_STRANDS, JG_ERR_UNSUPPORTED,
             "op %zu: pool-and-merge needs the frame rows of a translated window (not a strand program)", i);
  // the channels of the tensor it pools: what the last writer of the slot leaves (the two ops that keep the width: their input's)
  int buf = op.in_buf, channels = -1;
  for (size_t j = i; j-- > 0 && channels < 0;) {
    const jg_op &o = m->ops[j];
    if (!jg_op_writes(o, buf)) continue;
    if (o.kind == JG_OP_MAXPOOL1D || o.kind == JG_OP_FRAMESUM) buf = o.in_buf;
    else channels = o.cout;
  }
  JG_REQUIRE(channels == op.cout, JG_ERR_INVALID, "op %zu: pool-and-merge of %d channels, activation slot %d holds %d", i, op.cout,
             op.in_buf, channels);
  if (op.k != JG_POOLVEC_STORE) {
    bool written = false;
    for (size_t j = 0; j < i && !written; ++j) {
      const jg_op &o = m->ops[j];
      written = o.out_vec == op.out_vec && o.vec_off <= op.vec_off && o.vec_off + o.cout >= op.vec_off + op.cout &&
                (o.kind == JG_OP_POOLVEC || o.kind == JG_OP_POOL || o.kind == JG_OP_DENSE || o.kind == JG_OP_NMD_FINAL ||
                 o.kind == JG_OP_VECMAX || o.kind == JG_OP_OODSIG);
    }
    JG_REQUIRE(written, JG_ERR_INVALID, "op %zu: pool-and-merge %s into floats %d .. %d of vector slot %d, which no earlier op of the program wrote",
               i, op.k == JG_POOLVEC_ADD ? "adds" : "maximises", op.vec_off, op.vec_off + op.cout, op.out_vec);
  }
  JG_REQUIRE(op.n_stages == 0, JG_ERR_UNSUPPORTED, "op %zu: a pool-and-merge op carries no stages", i);
  return JG_OK;
}

static int validate_program(const jg_model *m, const float *weights) {
  int rc;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    auto slot_ok = [](int s, bool allow_ids) {
      return (s >= 0 && s < JG_MAX_BUFS) || s == JG_BUF_NONE || (allow_ids && s == JG_BUF_IDS);
    };
    JG_REQUIRE(op.kind >= JG_OP_CONV && op.kind <= JG_OP_POOLVEC, JG_ERR_INVALID,
               "op %zu: unknown kind %d", i, op.kind);
    if (op.kind == JG_OP_VECMAX)
      JG_REQUIRE(op.in_vec >= 0 && op.out_vec >= 0 && op.in_vec != op.out_vec && op.k >= 1 && op.cout >= 1 && op.vec_off >= 0,
                 JG_ERR_INVALID, "op %zu: vecmax takes k >= 1 groups of cout values from one vector into another", i);
    if (op.kind == JG_OP_STRANDS)
      JG_REQUIRE(i + 1 == m->ops.size() && op.k >= 2 && op.k <= 8 && op.arg >= JG_MERGE_AVERAGE && op.arg <= JG_MERGE_CONCAT,
                 JG_ERR_INVALID, "op %zu: a strands op closes the program, merges 2 - 8 strands by average / sum / max", i);
    JG_REQUIRE(slot_ok(op.in_buf, true) && slot_ok(op.out_buf, false) && slot_ok(op.in_mask, true) &&
                   slot_ok(op.out_mask, false),
               JG_ERR_INVALID, "op %zu: buffer slot out of range", i);
    JG_REQUIRE(op.in_vec >= -1 && op.in_vec < JG_MAX_VECS && op.out_vec >= -1 &&
                   op.out_vec < JG_MAX_VECS,
               JG_ERR_INVALID, "op %zu: vector slot out of range", i);
    JG_REQUIRE(op.n_stages >= 0 && op.n_stages <= JG_MAX_STAGES, JG_ERR_INVALID,
               "op %zu: %d stages", i, op.n_stages);
    auto off_ok = [&](int64_t off, int64_t n) { return off >= 0 && off + n <= m->n_w; };
    if (op.kind == JG_OP_CONV) {
      JG_REQUIRE(op.k >= 1 && op.cin >= 1 && op.cout >= 1 && op.stride >= 1 && op.dilation >= 1,
                 JG_ERR_INVALID, "op %zu: bad conv geometry", i);
      const int64_t cin_pad = (op.cin + 1) & ~1, cout_pad = (op.cout + 31) / 32 * 32;
      JG_REQUIRE(off_ok(op.w_off, (int64_t)op.k * cin_pad * cout_pad), JG_ERR_INVALID,
                 "op %zu: conv kernel outside the weight blob", i);
      if (op.in_buf == JG_BUF_IDS)
        JG_REQUIRE(off_ok(op.b_off, (int64_t)m->vocab * op.cin), JG_ERR_INVALID,
                   "op %zu: embedding table outside the weight blob", i);
    }
    if (op.kind == JG_OP_EMBED) {
      JG_REQUIRE(i == 0 && op.out_buf >= 0 && op.out_mask >= 0 && op.cout >= 4 && op.cout % 4 == 0 && m->vocab >= 2 &&
                     m->vocab <= 65536 && off_ok(op.b_off, (int64_t)m->vocab * op.cout),
                 JG_ERR_INVALID, "op %zu: an embedding op opens the program (vocabulary 2 .. 65536 - 16-bit ids above 256 -, table inside the weight blob)", i);
      // w_off >= 0: rows of a position table (k positions x cout floats) added to the looked-up rows
      JG_REQUIRE(op.w_off < 0 || (op.k >= 1 && off_ok(op.w_off, (int64_t)op.k * op.cout)), JG_ERR_INVALID,
                 "op %zu: position table outside the weight blob", i);
    } else if (!m->ops.empty() && m->ops[0].kind == JG_OP_EMBED) {
      JG_REQUIRE(op.in_buf != JG_BUF_IDS && op.in_mask != JG_BUF_IDS, JG_ERR_INVALID,
                 "op %zu: reads the id tensor directly in a program that opens with an embedding op (its buffer and mask take the tensor's place)", i);
    }
    if (jg_op_is_mixer(op.kind) && (rc = validate_mixer(m, i, weights)) != JG_OK) return rc;
    if (op.kind == JG_OP_MSMASK) {
      JG_REQUIRE(op.in_mask >= 0 && op.out_mask >= 0 && op.in_mask != op.out_mask, JG_ERR_INVALID,
                 "op %zu: a multi-scale mask op reads one mask slot and writes another", i);
      JgMsconvDesc d;
      if ((rc = msconv_desc(m, i, weights, &d)) != JG_OK) return rc;
    }
    if (op.kind == JG_OP_POOLVEC && (rc = validate_poolvec(m, i)) != JG_OK) return rc;
    if (op.kind == JG_OP_DENSE) {
      JG_REQUIRE(off_ok(op.w_off, (int64_t)op.cin * op.cout), JG_ERR_INVALID,
                 "op %zu: dense kernel outside the weight blob", i);
      JG_REQUIRE(op.b_off < 0 || off_ok(op.b_off, op.cout), JG_ERR_INVALID,
                 "op %zu: dense bias outside the weight blob", i);
    }
    {   // NMD taps per op: the conv kernels carry two accumulators, the element-wise / LayerNorm kernels one
      int n_nmd = 0;
      for (int s = 0; s < op.n_stages; ++s) n_nmd += op.stages[s].kind == JG_ST_NMD;
      JG_REQUIRE(n_nmd <= (op.kind == JG_OP_CONV ? 2 : 1), JG_ERR_UNSUPPORTED,
                 "op %zu: %d NMD taps in one stage list (at most %d)", i, n_nmd, op.kind == JG_OP_CONV ? 2 : 1);
    }
    for (int s = 0; s < op.n_stages; ++s) {
      const jg_stage &st = op.stages[s];
      const int64_t c = op.cout;
      switch (st.kind) {
        case JG_ST_BIAS:
          JG_REQUIRE(off_ok(st.p0, c), JG_ERR_INVALID, "op %zu stage %d: bias offset", i, s);
          break;
        case JG_ST_BN:
          JG_REQUIRE(off_ok(st.p0, c) && off_ok(st.p1, c) && off_ok(st.p2, c) && off_ok(st.p3, c),
                     JG_ERR_INVALID, "op %zu stage %d: batchnorm offsets", i, s);
          break;
        case JG_ST_DYT:
          JG_REQUIRE(off_ok(st.p2, c) && off_ok(st.p3, c), JG_ERR_INVALID,
                     "op %zu stage %d: dyt offsets", i, s);
          break;
        case JG_ST_ADD:
          JG_REQUIRE(st.arg >= 0 && st.arg < JG_MAX_BUFS, JG_ERR_INVALID,
                     "op %zu stage %d: add slot", i, s);
          break;
        case JG_ST_NMD:
          JG_REQUIRE(st.arg >= 0 && st.arg < JG_MAX_BUFS, JG_ERR_INVALID,
                     "op %zu stage %d: nmd partial slot", i, s);
          break;
        case JG_ST_LN:
          JG_REQUIRE(op.kind == JG_OP_ELTWISE && s == 0, JG_ERR_UNSUPPORTED,
                     "op %zu stage %d: a layer norm must lead an element-wise op", i, s);
          JG_REQUIRE(off_ok(st.p2, c) && off_ok(st.p3, c), JG_ERR_INVALID, "op %zu stage %d: layernorm offsets", i, s);
          break;
        case JG_ST_ACT:
        case JG_ST_MASKMUL:
          break;
        default:
          jg_set_error("op %zu stage %d: stage kind %d is not implemented", i, s, st.kind);
          return JG_ERR_UNSUPPORTED;
      }
    }
  }
  return JG_OK;
}

// The channel widths the conv, element-wise and LayerNorm kernels cover (a lane owns a channel quad; the LayerNorm kernel
// holds two quads per lane of a wave: 512 channels) - the limits jg_launch_conv, jg_launch_eltwise and jg_launch_layernorm
// require at every launch, named here so that a model outside them is refused when it is created, not in its first forward.
// An element-wise op is as wide as its cout (the shape walk holds its input to that).  The conv the table net replaces
// never reaches jg_launch_conv at rows the table covers and is left to the launch-time check at longer ones.
static int validate_widths(const jg_model *m) {
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    if (op.kind == JG_OP_CONV && (int)i != m->tab_conv)
      JG_REQUIRE(op.cin % 4 == 0 && op.cout % 4 == 0, JG_ERR_UNSUPPORTED,
                 "op %zu: conv of %d -> %d channels (both must be multiples of 4: a lane of the conv kernels owns a channel quad)", i,
                 op.cin, op.cout);
    if (op.kind != JG_OP_ELTWISE) continue;
    JG_REQUIRE(op.cout % 4 == 0, JG_ERR_UNSUPPORTED,
               "op %zu: element-wise op of %d channels (a multiple of 4: a lane of the kernel owns a channel quad)", i, op.cout);
    if (op.n_stages > 0 && op.stages[0].kind == JG_ST_LN)
      JG_REQUIRE(op.cout <= 512, JG_ERR_UNSUPPORTED,
                 "op %zu: layer norm over %d channels (up to 512: a lane of the kernel's wave holds two channel quads)", i, op.cout);
  }
  return JG_OK;
}

// The one shape walk: run the program at `l` positions per row and record what every op reads and writes (and check
// that the shapes line up).  Workspace sizes, FLOPs, tap shapes and the launchers of jg_run.hip all read these records.
int jg_shape_walk(const jg_model *m, int l, std::vector<OpShape> &shp) {
  Shape sh[JG_MAX_BUFS];
  int mL[JG_MAX_BUFS] = {}, vw[JG_MAX_VECS] = {};   // positions per frame of each mask slot, floats of each vector slot
  shp.assign(m->ops.size(), OpShape());
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    OpShape &r = shp[i];
    for (int q = 0; q < m->hprep[i].n_cvt; ++q) r.cvt[q] = sh[m->hprep[i].cvt_slot[q]];
    if (op.in_buf >= 0) r.in = sh[op.in_buf];
    switch (op.kind) {
      case JG_OP_CONV:
        if (op.in_buf == JG_BUF_IDS) r.in = Shape{m->id_frames, l, op.cin};
        JG_REQUIRE(r.in.C == op.cin, JG_ERR_INVALID, "op %zu: conv expects %d channels, input has %d", i, op.cin, r.in.C);
        conv_geometry(r.in.L, op.k, op.stride, op.dilation, op.padding, &r.L_out, &r.pad_left);
        JG_REQUIRE(r.L_out > 0, JG_ERR_INVALID, "op %zu: conv output is empty at %d codons per frame (window too short)", i, r.in.L);
        JG_REQUIRE(op.out_buf >= 0, JG_ERR_INVALID, "op %zu: conv needs an output slot", i);
        r.out = Shape{r.in.frames, r.L_out, op.cout};
        break;
      case JG_OP_EMBED:
        JG_REQUIRE(op.out_buf >= 0 && op.out_mask >= 0 && op.cout > 0, JG_ERR_INVALID, "op %zu: bad embedding op", i);
        JG_REQUIRE(op.w_off < 0 || l <= op.k, JG_ERR_UNSUPPORTED, "op %zu: rows of %d positions, the model's position table holds %d", i, l, op.k);
        r.out = Shape{m->id_frames, l, op.cout};
        r.m_out = l;
        break;
      case JG_OP_MASK:
        r.m_in = op.in_mask == JG_BUF_IDS ? l : mL[op.in_mask];
        conv_geometry(r.m_in, op.k, op.stride, op.dilation, op.padding, &r.L_out, &r.pad_left);
        JG_REQUIRE(op.out_mask >= 0 && r.L_out > 0, JG_ERR_INVALID, "op %zu: bad mask op", i);
        r.m_out = r.L_out;
        break;
      case JG_OP_MSMASK:
        r.m_in = mL[op.in_mask];
        JG_REQUIRE(r.m_in > 0, JG_ERR_INVALID, "op %zu: a multi-scale mask op on a mask slot nothing has written", i);
        r.L_out = r.m_out = r.m_in;      // padding same, strides 1
        break;
      case JG_OP_ELTWISE:
        JG_REQUIRE(r.in.C == op.cout, JG_ERR_INVALID, "op %zu: eltwise channel mismatch", i);
        r.out = r.in;
        break;
      case JG_OP_MAXPOOL1D:
        r.L_out = r.in.L / 2;
        JG_REQUIRE(r.L_out > 0, JG_ERR_INVALID, "op %zu: maxpool output empty", i);
        r.out = Shape{r.in.frames, r.L_out, r.in.C};
        break;
      case JG_OP_FRAMESUM: r.out = Shape{1, r.in.L, r.in.C}; break;
      case JG_OP_POOL:
        JG_REQUIRE(op.out_vec >= 0, JG_ERR_INVALID, "op %zu: pool needs an output vector", i);
        r.vec_need = op.vec_off + r.in.C;
        break;
      case JG_OP_POOLVEC:
        JG_REQUIRE(r.in.C == op.cout && r.in.frames >= 1 && r.in.frames <= JG_POOLVEC_MAX_FRAMES, JG_ERR_INVALID,
                   "op %zu: pool-and-merge of %d channels over (%d, L, %d) rows", i, op.cout, r.in.frames, r.in.C);
        if (op.in_mask >= 0) {
          r.m_in = mL[op.in_mask];
          JG_REQUIRE(r.m_in == r.in.L, JG_ERR_INVALID, "op %zu: pool-and-merge over rows of %d positions with a mask of %d", i, r.in.L, r.m_in);
        }
        r.vec_need = op.vec_off + op.cout;
        break;
      case JG_OP_DENSE:
        JG_REQUIRE(op.in_vec >= 0 && op.out_vec >= 0, JG_ERR_INVALID, "op %zu: dense vectors", i);
        JG_REQUIRE(vw[op.in_vec] >= op.cin, JG_ERR_INVALID, "op %zu: dense expects %d inputs, vector %d has %d", i, op.cin, op.in_vec, vw[op.in_vec]);
        r.vec_need = op.vec_off + op.cout;
        break;
      case JG_OP_NMD_FINAL:
        JG_REQUIRE(op.out_vec >= 0, JG_ERR_INVALID, "op %zu: nmd needs an output vector", i);
        r.vec_need = op.vec_off + op.cout;
        break;
      case JG_OP_OODSIG:
        JG_REQUIRE(op.out_vec >= 0, JG_ERR_INVALID, "op %zu: oodsig needs an output vector", i);
        r.vec_need = op.vec_off + op.cout;
        break;
      case JG_OP_VECMAX:
        JG_REQUIRE(vw[op.in_vec] >= op.k * op.cout, JG_ERR_INVALID, "op %zu: vecmax expects %d x %d inputs, vector %d has %d", i,
                   op.k, op.cout, op.in_vec, vw[op.in_vec]);
        r.vec_need = op.vec_off + op.cout;
        break;
      default: {
        if (!jg_op_is_mixer(op.kind)) break;
        const MixerKind &mk = *jg_mixer_kind(op.kind);
        const int frames = mk.six_frames ? 6 : m->id_frames;
        JG_REQUIRE(r.in.C == op.cin && r.in.frames == frames, JG_ERR_INVALID,
                   "op %zu: %s over %d channels expects (%d, L, %d) rows, input is (%d, L, %d)", i, mk.noun, op.cin, frames, op.cin, r.in.frames, r.in.C);
        if (mk.mask != MM_NONE && op.in_mask >= 0) {
          r.m_in = mL[op.in_mask];
          JG_REQUIRE(r.m_in == r.in.L, JG_ERR_INVALID, "op %zu: %s over rows of %d positions with a mask of %d", i, mk.noun, r.in.L, r.m_in);
        }
        if (mk.mask == MM_OWN && op.out_mask >= 0)
          JG_REQUIRE(mL[op.out_mask] == r.in.L, JG_ERR_INVALID, "op %zu: %s over rows of %d positions names an output mask of %d", i, mk.noun,
                     r.in.L, mL[op.out_mask]);
        if (op.kind == JG_OP_HYENA)
          JG_REQUIRE(r.in.L <= op.stride, JG_ERR_UNSUPPORTED,
                     "op %zu: hyena over rows of %d positions, the layer's filter table holds %d (seq_len of the layer, or the %d rows a program carries)",
                     i, r.in.L, op.stride, op.stride);
        r.scratch = (int64_t)r.in.frames * mixer_row_scratch(op, r.in.L);
        r.out = Shape{r.in.frames, r.in.L, op.cout};      // (of the same shape, but for the kind that widens)
      } break;
    }
    if (r.out.frames > 0) sh[op.out_buf] = r.out;
    if (r.m_out > 0) mL[op.out_mask] = r.m_out;
    if (r.vec_need > 0) vw[op.out_vec] = std::max(vw[op.out_vec], r.vec_need);
  }
  return JG_OK;
}

// Per-slot element counts (per window), vector widths and FLOPs per window: a fold over the shape records.
static void fold_shapes(const jg_model *m, int l, const std::vector<OpShape> &shp, int64_t act_elems[JG_MAX_BUFS],
                        int64_t msk_elems[JG_MAX_BUFS], int64_t nmd_elems[JG_MAX_BUFS], int vec_w[JG_MAX_VECS], double *flops) {
  for (int i = 0; i < JG_MAX_BUFS; ++i) act_elems[i] = msk_elems[i] = nmd_elems[i] = 0;
  for (int i = 0; i < JG_MAX_VECS; ++i) vec_w[i] = 0;
  const bool tab = jg_place_ctx(m, &shp, l).tab;
  double fl = 0.0;
  for (size_t i = 0; i < shp.size(); ++i) {
    const jg_op &op = m->ops[i];
    const OpShape &r = shp[i];
    if (op.kind == JG_OP_CONV) fl += 2.0 * op.k * op.cin * op.cout * (double)r.in.frames * r.L_out;
    if (jg_op_is_mixer(op.kind)) fl += jg_mixer_flops(m, i, r, 1);
    if (r.m_out > 0) msk_elems[op.out_mask] = std::max<int64_t>(msk_elems[op.out_mask], (int64_t)m->id_frames * r.m_out);
    if (r.vec_need > 0) vec_w[op.out_vec] = std::max(vec_w[op.out_vec], r.vec_need);
    if (r.out.frames == 0 || (tab && (int)i == m->tab_conv)) continue;      // (table net: the activation never exists)
    // (+ one position for an odd row: a phase-split tensor holds two phases of (L + 1) / 2 positions)
    const bool ps_room = op.kind == JG_OP_CONV || op.kind == JG_OP_EMBED || jg_op_is_mixer(op.kind);
    const Shape &t = r.out;
    act_elems[op.out_buf] = std::max<int64_t>(act_elems[op.out_buf], (int64_t)t.frames * (t.L + (ps_room ? t.L & 1 : 0)) * t.C);
    const int tiles = std::max((t.L + 63) / 64, 8 * ((t.L + 255) / 256));
    for (int s = 0; s < op.n_stages; ++s)                // an NMD tap of a conv or behind a LayerNorm: partial rows per tile
      if (op.stages[s].kind == JG_ST_NMD && (op.kind == JG_OP_CONV || op.kind == JG_OP_ELTWISE))
        nmd_elems[op.stages[s].arg] = std::max<int64_t>(nmd_elems[op.stages[s].arg], (int64_t)t.frames * tiles * t.C);
  }
  for (int i = 0; i < JG_MAX_VECS; ++i) vec_w[i] = (vec_w[i] + 3) & ~3;  // float4-aligned rows
  if (flops) *flops = fl;
}

extern "C" int jg_model_set_precision(jg_model *m, int mode) {
  JG_REQUIRE(m != nullptr && (mode == 0 || mode == 1), JG_ERR_INVALID, "jg_model_set_precision: bad args");
  if (mode == 1 && !m->f16_eligible) {
    jg_set_error("split-f16 path unavailable for this model: %s", m->f16_reason.c_str());
    return JG_ERR_UNSUPPORTED;
  }
  if (mode != m->precision) {
    JG_HIP(hipSetDevice(m->e->dev));
    JG_HIP(hipStreamSynchronize(m->e->stream));
    m->precision = mode;
  }
  return JG_OK;
}

extern "C" int jg_model_get_precision(const jg_model *m) { return m ? m->precision : -1; }

// One line per convolution: geometry, the kernel it runs on in mode 1 and, for the exact-f32 ones, why.
extern "C" int jg_model_describe(const jg_model *m, char *buf, int64_t cap) {
  JG_REQUIRE(m != nullptr && buf != nullptr && cap > 0, JG_ERR_INVALID, "jg_model_describe: bad arguments");
  std::string out;
  char line[512];
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    if (jg_op_is_mixer(op.kind)) {
      mixer_describe(op, i, line, sizeof(line));
      out += line;
      out += (m->f16_eligible && m->hprep[i].n_cvt > 0) ? " (F16S -> f32 conversion in front)\n" : "\n";
      continue;
    }
    if (op.kind == JG_OP_POOLVEC) {
      static const char *const pool_name[] = {"max", "average", "?", "last"}, *const merge_name[] = {"store", "add", "max"};
      snprintf(line, sizeof(line), "op %zu: pool-and-merge %s c=%d %s -> vector %d [%d, %d) %s x %g, one workgroup a window, f32 rows\n", i,
               pool_name[op.arg & 3], op.cout, op.in_mask >= 0 ? "masked" : "no mask", op.out_vec, op.vec_off, op.vec_off + op.cout,
               merge_name[op.k % 3], (double)op.f0);
      out += line;
      continue;
    }
    if (op.kind != JG_OP_CONV) continue;
    const ConvHPrep &hp = m->hprep[i];
    const Place pl = jg_place_op(m, i, jg_place_nominal());   // (no row length: a small-window model answers for its 500-bp rows)
    const char *where = m->small != nullptr ? "fused small-window kernel"
                        : pl == PL_RB_CONV1 ? "split-f16 (fused residual block: computed by the block's second conv)"
                        : (pl == PL_RB32 || pl == PL_RB64) ? (hp.ps_store ? "split-f16 (fused residual block, phase-split store)" : "split-f16 (fused residual block)")
                        : pl != PL_CONV_F16 ? "exact-f32"
                        : hp.d_lut != nullptr ? "split-f16 (table lookup)"
                        : hp.ps_read == 1 ? "split-f16 (stride 2 as a 3-tap conv over the two phases of its phase-split input)"
                        : hp.ps_read == 2 ? "split-f16 (stride 2 on the even phase of its phase-split input)"
                        : hp.ps_store ? (hp.cw != 128 ? "split-f16 (narrow tile, phase-split store)" : "split-f16 (phase-split store)")
                        : hp.as_k5 ? "split-f16 (tap range of the 5-tap kernel)"
                        : hp.cw != 128 ? "split-f16 (narrow tile)" : "split-f16";
    const bool say_why = !jg_place_is_f16(pl) && m->small == nullptr;
    static const char *const st_name[] = {"?", "bias", "bn", "dyt", "add", "act", "nmd", "maskmul", "ln"};
    std::string stages;
    for (int q = 0; q < op.n_stages; ++q) {
      const int kd = op.stages[q].kind;
      stages += (q ? " " : "");
      stages += (kd >= 1 && kd <= 8) ? st_name[kd] : "?";
    }
    snprintf(line, sizeof(line), "op %zu: conv k=%d cin=%d cout=%d stride=%d dilation=%d [%s] -> %s%s%s\n", i, op.k, op.cin,
             op.cout, op.stride, op.dilation, stages.c_str(), where,
             (say_why && !hp.why_f32.empty()) ? ": " : "", say_why ? hp.why_f32.c_str() : "");
    out += line;
  }
  const size_t n = std::min(out.size(), (size_t)cap - 1);
  memcpy(buf, out.data(), n);
  buf[n] = 0;
  return JG_OK;
}

extern "C" int64_t jg_model_get_stat(const jg_model *m, int key) {
  if (m == nullptr) return -1;
  int64_t n_conv = 0, n_f16 = 0, n_cvt = 0;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    n_cvt += m->hprep[i].n_cvt;
    if (m->ops[i].kind != JG_OP_CONV) continue;
    ++n_conv;
    n_f16 += jg_place_is_f16(jg_place_op(m, i, jg_place_nominal())) ? 1 : 0;
  }
  switch (key) {
    case JG_MSTAT_CONVS: return n_conv;
    case JG_MSTAT_CONVS_F16X3: return n_f16;
    case JG_MSTAT_LAYOUT_CONVERSIONS: return m->f16_eligible ? n_cvt : 0;
    case JG_MSTAT_SMALL_FUSED: return m->small != nullptr ? 1 : 0;
    case JG_MSTAT_TAP_VARIANT: return m->tap_variant;
    case JG_MSTAT_TAP_INSTANCE: return jg_conv_inst_get(m, -1, false);
    case JG_MSTAT_TAP_INSTANCE_OTHER: return jg_conv_inst_get(m, -1, true);
    case JG_MSTAT_OPERAND_DIGEST: return jg_operand_digest(m);
    default:
      if (key >= JG_MSTAT_CONV_INSTANCE0 && key < JG_MSTAT_CONV_INSTANCE0 + (int)m->ops.size())
        return jg_conv_inst_get(m, key - JG_MSTAT_CONV_INSTANCE0, false);
      return -1;
  }
}

extern "C" int jg_model_destroy(jg_model *m);
extern "C" int jg_model_create(jg_engine *e, const jg_op *ops, int n_ops, const float *weights,
                               int64_t n_weights, int32_t vocab, jg_model **out) {
  JG_REQUIRE(e != nullptr && ops != nullptr && n_ops > 0 && weights != nullptr && n_weights > 0 &&
                 out != nullptr,
             JG_ERR_INVALID, "jg_model_create: bad arguments");
  JG_HIP(hipSetDevice(e->dev));
  jg_model *m = new jg_model();
  m->e = e;
  m->ops.assign(ops, ops + n_ops);
  m->n_w = n_weights;
  m->vocab = vocab;
  int rc = validate_program(m, weights);
  if (rc != JG_OK) { delete m; return rc; }
  if (m->ops[0].kind == JG_OP_EMBED && m->vocab > 256) m->id_bytes = 2;
  if (m->ops.back().kind == JG_OP_STRANDS) {
    m->strands = m->ops.back().k;
    m->id_frames = 1;
    m->merge_kind = m->ops.back().arg;
  }
  hipError_t err = hipMalloc(&m->d_w, (size_t)n_weights * sizeof(float));
  if (err != hipSuccess) {
    jg_set_error("jg_model_create: weights hipMalloc -> %s", hipGetErrorString(err));
    delete m;
    return JG_ERR_NOMEM;
  }
  JG_HIP(hipMemcpy(m->d_w, weights, (size_t)n_weights * sizeof(float), hipMemcpyHostToDevice));
  JG_HIP(hipMalloc(&m->d_lut, 80));
  JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->d_overflow), sizeof(int)));
  JG_HIP(hipMemset(m->d_overflow, 0, sizeof(int)));
  rc = jg_prepare_tab(m, weights);
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  rc = validate_widths(m);                          // (behind jg_prepare_tab: the table net takes the conv it replaces)
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  rc = jg_prepare_f16(m, weights);
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  for (size_t i = 0; i < m->ops.size(); ++i) {      // (behind jg_prepare_f16: it sizes the per-op records)
    JgMsconvDesc d;
    if (m->ops[i].kind != JG_OP_MSCONV) continue;
    if ((rc = msconv_desc(m, i, weights, &d)) != JG_OK) { jg_model_destroy(m); return rc; }
    m->hprep[i].ms_halo_l = d.halo_l; m->hprep[i].ms_halo_r = d.halo_r; m->hprep[i].ms_macs = d.macs;
  }
  rc = jg_plan_phase_split(m, weights);
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  rc = jg_plan_resblocks(m, weights);
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  rc = jg_prepare_f32(m, weights);
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  // the 32-channel small-window family has a fused kernel of its own (same split-f16 arithmetic): where the program
  // matches it, it takes precedence over the layer-by-layer placement above (whose narrow-conv kernels would run the
  // same model several times slower)
  rc = jg_prepare_small(m, weights);
  if (rc != JG_OK) { jg_model_destroy(m); return rc; }
  if (m->small != nullptr) m->f16_eligible = true;
  m->precision = m->f16_eligible ? 1 : 0;
  *out = m;
  return JG_OK;
}

static void free_workspace(jg_model *m) {
  for (int i = 0; i < JG_MAX_BUFS; ++i) {
    if (m->act[i]) (void)hipFree(m->act[i]);
    if (m->msk[i]) (void)hipFree(m->msk[i]);
    if (m->nmd_part[i]) (void)hipFree(m->nmd_part[i]);
    m->act[i] = nullptr; m->msk[i] = nullptr; m->nmd_part[i] = nullptr;
    m->act_cap[i] = m->msk_cap[i] = m->nmd_cap[i] = 0;
  }
  for (int i = 0; i < JG_MAX_VECS; ++i) {
    if (m->vec[i]) (void)hipFree(m->vec[i]);
    m->vec[i] = nullptr;
    m->vec_cap[i] = 0;
  }
  if (m->cvt_scratch) (void)hipFree(m->cvt_scratch);
  m->cvt_scratch = nullptr;
  m->cvt_cap = 0;
  if (m->tap_buf) (void)hipFree(m->tap_buf);
  m->tap_buf = nullptr;
  m->tap_cap = 0;
}

extern "C" int jg_model_destroy(jg_model *m) {
  if (m == nullptr) return JG_OK;
  (void)hipSetDevice(m->e->dev);
  (void)hipStreamSynchronize(m->e->stream);
  jg_conv_inst_reset(m);
  free_workspace(m);
  jg_free_small(m);
  for (int i = 0; i < JG_MAX_VECS; ++i)
    if (m->merged[i]) (void)hipFree(m->merged[i]);
  if (m->tab_wfrag) (void)hipFree(m->tab_wfrag);
  if (m->tab_bias512) (void)hipFree(m->tab_bias512);
  if (m->tab_table) (void)hipFree(m->tab_table);
  if (m->tab_bias) (void)hipFree(m->tab_bias);
  if (m->d_w) (void)hipFree(m->d_w);
  if (m->hy_scratch) (void)hipFree(m->hy_scratch);
  if (m->d_ids) (void)hipFree(m->d_ids);
  if (m->d_counts) (void)hipFree(m->d_counts);
  if (m->d_win) (void)hipFree(m->d_win);
  if (m->d_bases_buf) (void)hipFree(m->d_bases_buf);
  if (m->d_lut) (void)hipFree(m->d_lut);
  if (m->d_overflow) (void)hipFree(m->d_overflow);
  if (m->pool_part) (void)hipFree(m->pool_part);
  for (auto &hp : m->hprep) {
    if (hp.d_wh) (void)hipFree(hp.d_wh);
    for (int par = 0; par < 2; ++par) if (hp.d_wh_ps[par]) (void)hipFree(hp.d_wh_ps[par]);
    if (hp.d_rb_wfrag) (void)hipFree(hp.d_rb_wfrag);
    if (hp.d_rb_epi) (void)hipFree(hp.d_rb_epi);
    if (hp.d_embh) (void)hipFree(hp.d_embh);
    if (hp.d_epi) (void)hipFree(hp.d_epi);
    if (hp.d_w8) (void)hipFree(hp.d_w8);
    if (hp.d_lut) (void)hipFree(hp.d_lut);
    if (hp.d_epi_lut) (void)hipFree(hp.d_epi_lut);
  }
  delete m;
  return JG_OK;
}

// Workspace for `chunk` windows of `l` codons per frame.  Buffers are kept as long as they are large enough
// (the short-contig pass calls with a different l for every batch: commands/predict.py:236-245), and grow to the
// largest request seen.
int jg_ensure_workspace(jg_model *m, int64_t chunk, int l, const std::vector<OpShape> &shp) {
  int64_t nmd_elems[JG_MAX_BUFS];
  fold_shapes(m, l, shp, m->act_elems, m->msk_elems, nmd_elems, m->vec_w, nullptr);
  int64_t hy_need = 0;                 // the hyena ops' projection scratch: kept apart from the slots, grown on demand
  for (const OpShape &r : shp) hy_need = std::max(hy_need, chunk * r.scratch * (int64_t)sizeof(float));
  if (hy_need > m->hy_cap) {
    JG_HIP(hipStreamSynchronize(m->e->stream));
    int rc = grow(&m->hy_scratch, &m->hy_cap, hy_need);
    if (rc != JG_OK) return rc;
  }
  bool fits = true;
  for (int i = 0; i < JG_MAX_BUFS; ++i) {
    m->nmd_part_elems[i] = nmd_elems[i];
    fits &= chunk * m->act_elems[i] <= m->act_cap[i] && chunk * m->msk_elems[i] <= m->msk_cap[i] &&
            chunk * nmd_elems[i] <= m->nmd_cap[i];
  }
  for (int i = 0; i < JG_MAX_VECS; ++i) fits &= chunk * m->vec_w[i] <= m->vec_cap[i];
  // programs with layout conversions swap a slot's tensor with the scratch tensor: every activation slot and the
  // scratch then need the LARGEST slot's size (a smaller buffer would otherwise wander into a larger slot - found by
  // the architecture fuzz on a net with two strided blocks)
  int64_t cvt_need = 0;
  if (m->needs_cvt) {
    for (int i = 0; i < JG_MAX_BUFS; ++i) cvt_need = std::max(cvt_need, chunk * m->act_elems[i]);
    for (int i = 0; i < JG_MAX_BUFS; ++i)
      if (m->act_elems[i] > 0) fits &= cvt_need <= m->act_cap[i];
  }
  fits &= cvt_need <= m->cvt_cap;
  if (fits) return JG_OK;
  JG_HIP(hipStreamSynchronize(m->e->stream));
  int64_t want_act[JG_MAX_BUFS], want_msk[JG_MAX_BUFS], want_nmd[JG_MAX_BUFS], want_vec[JG_MAX_VECS];
  for (int i = 0; i < JG_MAX_BUFS; ++i) {
    want_act[i] = std::max(m->act_cap[i], chunk * m->act_elems[i]);
    if (m->needs_cvt && m->act_elems[i] > 0) want_act[i] = std::max(want_act[i], cvt_need);
    want_msk[i] = std::max(m->msk_cap[i], chunk * m->msk_elems[i]);
    want_nmd[i] = std::max(m->nmd_cap[i], chunk * nmd_elems[i]);
  }
  for (int i = 0; i < JG_MAX_VECS; ++i) want_vec[i] = std::max(m->vec_cap[i], chunk * (int64_t)m->vec_w[i]);
  const int64_t want_cvt = std::max(m->cvt_cap, cvt_need);
  free_workspace(m);
  if (want_cvt > 0) {
    JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->cvt_scratch), (size_t)want_cvt * sizeof(float)));
    m->cvt_cap = want_cvt;
  }
  for (int i = 0; i < JG_MAX_BUFS; ++i) {
    if (want_act[i] > 0) JG_HIP(hipMalloc(&m->act[i], (size_t)want_act[i] * sizeof(float)));
    if (want_msk[i] > 0) JG_HIP(hipMalloc(&m->msk[i], (size_t)want_msk[i]));
    if (want_nmd[i] > 0) JG_HIP(hipMalloc(&m->nmd_part[i], (size_t)want_nmd[i] * sizeof(float)));
    m->act_cap[i] = want_act[i]; m->msk_cap[i] = want_msk[i]; m->nmd_cap[i] = want_nmd[i];
  }
  for (int i = 0; i < JG_MAX_VECS; ++i)
    if (want_vec[i] > 0) {
      JG_HIP(hipMalloc(&m->vec[i], (size_t)want_vec[i] * sizeof(float)));
      JG_HIP(hipMemsetAsync(m->vec[i], 0, (size_t)want_vec[i] * sizeof(float), m->e->stream));
      m->vec_cap[i] = want_vec[i];
    }
  return JG_OK;
}

// ---- test readback (jg_model_set_tap) ---------------------------------------------------------------------------
// why op i's output is never stored under placement c (rows of l positions when c has a row length), or nullptr
const char *jg_tap_refusal(const jg_model *m, size_t i, const PlaceCtx &c, int l, char *why, size_t cap) {
  const jg_op &op = m->ops[i];
  if (op.kind != JG_OP_CONV && op.kind != JG_OP_MASK && op.kind != JG_OP_MSMASK && op.kind != JG_OP_ELTWISE && op.kind != JG_OP_EMBED &&
      op.kind != JG_OP_MAXPOOL1D && op.kind != JG_OP_FRAMESUM && !jg_op_is_mixer(op.kind)) {
    snprintf(why, cap, "op %zu (kind %d) writes a vector or nothing - pool, dense and vector results are outputs already", i, op.kind);
    return why;
  }
  const ConvHPrep &hp = m->hprep[i];
  switch (jg_place_op(m, i, c)) {
    case PL_SMALL_SKIP:
      snprintf(why, cap, "op %zu runs inside the fused small-window kernel at rows of %d positions (no tensor is stored)", i, l);
      return why;
    case PL_TAB_CONV:
      snprintf(why, cap, "op %zu runs inside the table-net strand kernel (conv + pool in one launch, no tensor is stored)", i);
      return why;
    case PL_RB_CONV1:
      snprintf(why, cap, "op %zu is conv1 of a fused residual block: op %d computes it in LDS and stores only the block's "
               "output (engine option JG_OPT_FUSE_RESBLOCK 0 exposes it)", i, hp.rb_second);
      return why;
    case PL_CONV_F16:
      if (hp.pool_op < 0) return nullptr;
      snprintf(why, cap, "op %zu is store-free: its only reader, the masked max pool op %d, is fused into its epilogue", i, hp.pool_op);
      return why;
    default:
      return nullptr;
  }
}

// copy the tensor op i just wrote (r: its shape record, c: the run's placement) into the tap's host destination
int jg_tap_copy(jg_model *m, size_t i, const OpShape &r, const PlaceCtx &c, int nw, hipStream_t s) {
  const jg_op &op = m->ops[i];
  uint8_t *dst = static_cast<uint8_t *>(m->tap_dst);
  if (op.kind == JG_OP_MASK || op.kind == JG_OP_MSMASK) {
    const int64_t per_row = (int64_t)m->id_frames * r.m_out;         // frames x L_out bytes per program row
    JG_REQUIRE((m->tap_row0 + nw) * per_row <= m->tap_bytes, JG_ERR_INVALID, "tap: destination of %lld bytes too small",
               (long long)m->tap_bytes);
    JG_HIP(hipMemcpyAsync(dst + m->tap_row0 * per_row, m->msk[op.out_mask], (size_t)(nw * per_row), hipMemcpyDeviceToHost, s));
    JG_HIP(hipStreamSynchronize(s));
    return JG_OK;
  }
  const Shape t = r.out;
  const int64_t per_row = (int64_t)t.frames * t.L * t.C * (int64_t)sizeof(float);
  const int64_t rows = (int64_t)nw * t.frames;
  JG_REQUIRE((m->tap_row0 + nw) * per_row <= m->tap_bytes, JG_ERR_INVALID, "tap: destination of %lld bytes too small",
             (long long)m->tap_bytes);
  // the slot's layout, from the placement and the format plan
  const ConvHPrep &hp = m->hprep[i];
  const Place pl = jg_place_op(m, i, c);
  const bool rb = pl == PL_RB32 || pl == PL_RB64, f16_conv = rb || pl == PL_CONV_F16;
  const bool psplit = f16_conv && hp.ps_store;
  const bool f16s = psplit || rb || (f16_conv && hp.out_f16s) || (op.kind == JG_OP_MAXPOOL1D && c.prec == 1 && hp.pool_f16s);
  int64_t v = 0;
  if (f16s) v |= JG_TAP_F16S;
  if (psplit) v |= JG_TAP_PHASE_SPLIT;
  if (rb) v |= JG_TAP_FUSED_RESBLOCK;
  if (pl == PL_CONV_F32) v |= JG_TAP_EXACT_F32;
  if (pl == PL_CONV_F16 && m->tap_flat) v |= JG_TAP_WINDOW_PACKED;
  if (f16_conv && hp.d_lut != nullptr) v |= JG_TAP_TABLE_LOOKUP;
  if (f16_conv && hp.cw != 128) v |= JG_TAP_NARROW;
  if (jg_op_is_mixer(op.kind)) v |= JG_TAP_EXACT_F32;      // one arithmetic (exact-f32 matrix cores), one layout (f32 rows)
  m->tap_variant |= v;
  float *out = reinterpret_cast<float *>(dst + m->tap_row0 * per_row);
  if (!f16s) {
    JG_HIP(hipMemcpyAsync(out, m->act[op.out_buf], (size_t)(nw * per_row), hipMemcpyDeviceToHost, s));
    JG_HIP(hipStreamSynchronize(s));
    return JG_OK;
  }
  // F16S [rows][C/16][hi|lo][2][L] -> f32 (rows, L, C); a phase-split tensor is an F16S tensor of (L + 1) / 2 positions
  // and 2C channels (position p of channel c at position p / 2, channel (p & 1) C + c)
  const int L2 = psplit ? (t.L + 1) / 2 : t.L, C2 = psplit ? 2 * t.C : t.C;
  const int64_t need = rows * L2 * (int64_t)C2 * (int64_t)sizeof(float);
  int rc = grow(&m->tap_buf, &m->tap_cap, need);
  if (rc != JG_OK) return rc;
  if ((rc = jg_launch_f16s_to_f32(reinterpret_cast<const uint4 *>(m->act[op.out_buf]), rows, L2, C2, m->tap_buf, s)) != JG_OK)
    return rc;
  if (!psplit) {
    JG_HIP(hipMemcpyAsync(out, m->tap_buf, (size_t)need, hipMemcpyDeviceToHost, s));
    JG_HIP(hipStreamSynchronize(s));
    return JG_OK;
  }
  std::vector<float> tmp((size_t)(need / sizeof(float)));
  JG_HIP(hipMemcpyAsync(tmp.data(), m->tap_buf, (size_t)need, hipMemcpyDeviceToHost, s));
  JG_HIP(hipStreamSynchronize(s));
  for (int64_t r = 0; r < rows; ++r)
    for (int p = 0; p < t.L; ++p)
      memcpy(out + (r * t.L + p) * t.C, tmp.data() + (r * L2 + p / 2) * C2 + (p & 1) * t.C, (size_t)t.C * sizeof(float));
  return JG_OK;
}

extern "C" int jg_model_tap_shape(const jg_model *m, int op, int32_t l, int64_t shape[4]) {
  JG_REQUIRE(m != nullptr && shape != nullptr && l > 0 && op >= 0 && op < (int)m->ops.size(), JG_ERR_INVALID,
             "jg_model_tap_shape: bad arguments");
  for (int q = 0; q < 4; ++q) shape[q] = 0;
  std::vector<OpShape> shp;
  int rc = jg_shape_walk(m, l, shp);
  if (rc != JG_OK) return rc;
  const OpShape &r = shp[(size_t)op];                   // the tensor this op wrote, per window
  shape[0] = m->strands;
  if (m->ops[(size_t)op].kind == JG_OP_MASK || m->ops[(size_t)op].kind == JG_OP_MSMASK) {
    shape[1] = m->id_frames; shape[2] = r.m_out; shape[3] = 1;
  } else {
    shape[1] = r.out.frames; shape[2] = r.out.L; shape[3] = r.out.C;
  }
  JG_REQUIRE(shape[1] > 0, JG_ERR_UNSUPPORTED, "jg_model_tap_shape: op %d (kind %d) writes no tensor", op, m->ops[(size_t)op].kind);
  return JG_OK;
}

extern "C" int jg_model_set_tap(jg_model *m, int op, void *host_dst, int64_t dst_bytes) {
  JG_REQUIRE(m != nullptr && op >= -1 && op < (int)m->ops.size(), JG_ERR_INVALID, "jg_model_set_tap: bad arguments");
  if (op >= 0) {
    JG_REQUIRE(host_dst != nullptr && dst_bytes > 0, JG_ERR_INVALID, "jg_model_set_tap: no destination");
    char why[256];
    if (jg_tap_refusal(m, (size_t)op, jg_place_ctx(m, nullptr, 0), 0, why, sizeof(why)) != nullptr) {
      jg_set_error("jg_model_set_tap: %s", why);
      return JG_ERR_UNSUPPORTED;
    }
  }
  m->tap_op = op;
  m->tap_dst = op >= 0 ? host_dst : nullptr;
  m->tap_bytes = op >= 0 ? dst_bytes : 0;
  if (op >= 0) m->tap_variant = 0;                    // (turning the tap off keeps the last forward's bits readable)
  return JG_OK;
}

extern "C" int jg_model_vec_width(const jg_model *m, int which) {
  if (m == nullptr || which < 0 || which > 3) return 0;
  // slot convention: 0 embedding, 1 nmd, 2 prediction, 3 reliability
  static const int slot_of[4] = {2, 3, 0, 1};
  // unpadded widths: recompute from the ops
  int width = 0;
  const int slot = slot_of[which];
  for (const jg_op &op : m->ops) {
    if (op.out_vec != slot) continue;
    int wd = 0;
    if (op.kind == JG_OP_DENSE || op.kind == JG_OP_NMD_FINAL || op.kind == JG_OP_VECMAX || op.kind == JG_OP_POOL || op.kind == JG_OP_POOLVEC) wd = op.vec_off + op.cout;
    width = std::max(width, wd);
  }
  // a branched model whose classifier's merge layer is Concatenate (builder.py:1262-1265): the window's prediction is the
  // strands' head outputs side by side
  if (which == 0 && m->strands > 1 && m->merge_kind == JG_MERGE_CONCAT) width *= m->strands;
  return width;
}

extern "C" double jg_model_flops_per_window(const jg_model *m, int32_t l) {
  if (m == nullptr) return 0.0;
  int64_t a[JG_MAX_BUFS], b[JG_MAX_BUFS], c[JG_MAX_BUFS];
  int vw[JG_MAX_VECS];
  double fl = 0.0;
  std::vector<OpShape> shp;
  if (jg_shape_walk(m, l, shp) != JG_OK) return 0.0;
  fold_shapes(m, l, shp, a, b, c, vw, &fl);
  return fl;
}
