// Model preparation (host): which kernels the op program matches, and their operands - the table net, the split-f16 and
// exact-f32 conv operands, phase-split tensors, fused residual blocks, the small-window network.  jg_model_create
// (jg_model.hip) calls them in this order; what they decide is read back through jg_place_op (jg_run.hip).
#include "jg_host.h"


// ---------------------------------------------------------------------------
// split-f16 operand preparation (host): see jg_conv_f16.hip for the layouts
// ---------------------------------------------------------------------------
static inline uint16_t f16_bits(float x) {
  _Float16 h = (_Float16)x;
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}
static inline float f16_value(float x) { return (float)(_Float16)x; }

// ---------------------------------------------------------------------------
// fused small-window network (jg_small.hip): does the op program match the family, and its operands
//   [MASK] CONV(ids, k0, E -> 32)  { [MASK] CONV(k 3, 32 -> 32, SAME) } x 2 | 4   POOL(avg | max)   ...heads
// every conv's stages being  [BIAS] [BN]  [ADD]  GELU(tanh)  [ [BN] GELU(tanh) ]
// ---------------------------------------------------------------------------
void jg_free_small(jg_model *m) {
  if (m->small == nullptr) return;
  JgSmallNet *sn = m->small;
  if (sn->d_lut) (void)hipFree(sn->d_lut);
  if (sn->d_epi) (void)hipFree(sn->d_epi);
  if (sn->d_part) (void)hipFree(sn->d_part);
  if (sn->d_wfrag) (void)hipFree(sn->d_wfrag);
  delete sn;
  m->small = nullptr;
}

int jg_prepare_small(jg_model *m, const float *weights) {
  std::vector<int> convs;
  int pool_op = -1;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    if (op.kind == JG_OP_MASK || op.kind == JG_OP_NMD_FINAL) continue;     // (NMD finishes: matched to taps below)
    if (op.kind == JG_OP_CONV) { convs.push_back((int)i); continue; }
    if (op.kind == JG_OP_POOL) { pool_op = (int)i; break; }
    return JG_OK;                                   // anything else in front of the pool: not this family
  }
  const int nc = (int)convs.size() - 1;
  if (pool_op < 0 || nc < 1 || !jg_small_supports(nc, m->ops[convs[0]].k, m->vocab)) return JG_OK;
  const jg_op &c0 = m->ops[convs[0]];
  if (c0.in_buf != JG_BUF_IDS || c0.cout != 32 || c0.stride != 1 || c0.dilation != 1 || c0.mask_mode != JG_MASK_ANY ||
      !(c0.in_mask == JG_BUF_IDS || c0.in_mask == JG_BUF_NONE))
    return JG_OK;
  const bool use_mask = c0.in_mask == JG_BUF_IDS;
  for (int q = 1; q <= nc; ++q) {
    const jg_op &c = m->ops[convs[q]];
    if (c.in_buf != m->ops[convs[q - 1]].out_buf || c.k != 3 || c.cin != 32 || c.cout != 32 || c.stride != 1 ||
        c.dilation != 1 || c.padding != JG_PAD_SAME || c.mask_mode != JG_MASK_ANY || (c.in_mask >= 0) != use_mask)
      return JG_OK;
    if (use_mask && c.in_mask != m->ops[convs[q - 1]].out_mask) return JG_OK;
  }
  const jg_op &pl = m->ops[pool_op];
  if (pl.in_buf != m->ops[convs[nc]].out_buf || !(pl.arg == JG_POOL_AVG || pl.arg == JG_POOL_MAX) ||
      (pl.in_mask >= 0) != use_mask || (use_mask && pl.in_mask != m->ops[convs[nc]].out_mask))
    return JG_OK;
  // no later op may read an activation slot (the kernel never writes them)
  for (size_t i = (size_t)pool_op + 1; i < m->ops.size(); ++i) {
    const int k = m->ops[i].kind;
    if (k == JG_OP_CONV || k == JG_OP_MASK || k == JG_OP_POOL || k == JG_OP_ELTWISE || k == JG_OP_MAXPOOL1D ||
        k == JG_OP_FRAMESUM || k == JG_OP_NMD_FINAL || jg_op_is_mixer(k))
      return JG_OK;
  }
  JgSmallNet *sn = new JgSmallNet();
  for (JgSmallLayer &ly : sn->layer) ly.add = ly.aff2 = ly.save = ly.tap = 0;
  std::vector<float> epi((size_t)(nc + 1) * 4 * 32, 0.f);
  bool ok = true;
  // split-f16 weight fragments of the k = 3 convs: built behind the fold below (the first affine's scale goes into them)
  std::vector<uint16_t> frag((size_t)nc * 12 * 64 * 8, 0);
  std::vector<double> scale1((size_t)(nc + 1) * 32, 1.0), shift1((size_t)(nc + 1) * 32, 0.0);
  // epilogue parameters: fold BIAS / BN chains (f64), match  affine [ADD] GELU [affine GELU]
  for (int q = 0; q <= nc && ok; ++q) {
    const jg_op &c = m->ops[convs[q]];
    std::vector<double> s1(32, 1.0), t1(32, 0.0), s2(32, 1.0), t2(32, 0.0);
    int st = 0;
    auto fold = [&](std::vector<double> &sc, std::vector<double> &sh) {
      bool any = false;
      for (; st < c.n_stages; ++st) {
        const jg_stage &g = c.stages[st];
        if (g.kind == JG_ST_BIAS) {
          for (int n = 0; n < 32; ++n) sh[n] += (double)weights[g.p0 + n];
        } else if (g.kind == JG_ST_BN) {
          for (int n = 0; n < 32; ++n) {
            const double mu = weights[g.p0 + n], is = weights[g.p1 + n], ga = weights[g.p2 + n], be = weights[g.p3 + n];
            sc[n] = sc[n] * is * ga;
            sh[n] = (sh[n] - mu) * is * ga + be;
          }
        } else break;
        any = true;
      }
      return any;
    };
    fold(s1, t1);
    JgSmallLayer &ly = sn->layer[q];
    if (st < c.n_stages && c.stages[st].kind == JG_ST_ADD) {
      // the shortcut must be the output of an earlier layer of this chain, and the only one alive
      int src = -1;
      for (int r = q - 1; r >= 0; --r)
        if (m->ops[convs[r]].out_buf == c.stages[st].arg) { src = r; break; }
      if (src < 0) { ok = false; break; }
      bool clobbered = false;
      for (int r = src + 1; r < q; ++r) clobbered |= m->ops[convs[r]].out_buf == c.stages[st].arg;
      if (clobbered) { ok = false; break; }
      sn->layer[src].save = 1;
      ly.add = 1;
      ++st;
    }
    if (!(st < c.n_stages && c.stages[st].kind == JG_ST_ACT && c.stages[st].arg == JG_ACT_GELU_TANH)) { ok = false; break; }
    ++st;
    if (st < c.n_stages && (c.stages[st].kind == JG_ST_BIAS || c.stages[st].kind == JG_ST_BN)) {
      fold(s2, t2);
      if (!(st < c.n_stages && c.stages[st].kind == JG_ST_ACT && c.stages[st].arg == JG_ACT_GELU_TANH)) { ok = false; break; }
      ++st;
      ly.aff2 = 1;
      // (the first layer's accumulators come out of the table phase and its epilogue has no second affine: jg_small.hip)
      if (q == 0) { ok = false; break; }
    }
    if (st < c.n_stages && c.stages[st].kind == JG_ST_NMD && st == c.n_stages - 1) {
      // a tap behind the layer's last stage: masked channel sums of the layer's output, finished by the NMD_FINAL op
      // that reads this partial slot (the program's slot number is kept to find it)
      ly.tap = ++sn->n_taps;
      sn->tap_part_slot[ly.tap] = c.stages[st].arg;
      sn->tap_conv_op[ly.tap] = convs[q];
      ++st;
    }
    if (st != c.n_stages) { ok = false; break; }
    for (int n = 0; n < 32; ++n) {
      // the first affine lives in the weights (scale) and in the accumulators' initial value (shift): jg_small.hip
      scale1[(size_t)q * 32 + n] = s1[n];
      shift1[(size_t)q * 32 + n] = t1[n];
      epi[((size_t)q * 4 + 0) * 32 + n] = 1.0f;
      epi[((size_t)q * 4 + 1) * 32 + n] = (float)t1[n];
      epi[((size_t)q * 4 + 2) * 32 + n] = (float)s2[n];
      epi[((size_t)q * 4 + 3) * 32 + n] = (float)t2[n];
    }
  }
  for (int q = 1; q <= nc && ok; ++q) {
    const jg_op &c = m->ops[convs[q]];
    const float *w = weights + c.w_off;               // (3, 32, 32) f32 (cin even, cout multiple of 32: no padding)
    // the folded weights w * scale1 go into f16 planes WITHOUT a power-of-two pre-scale: they must sit inside the f16
    // range (a large batch-norm scale would turn hi into inf and lo into -inf: NaN logits), and the layer's largest
    // weight must stay well above the subnormal quantum 2^-24 the lo plane resolves (hi + lo then still carries ~19 bits of
    // it); otherwise the model stays on the generic split-f16 / exact-f32 kernels, which pre-scale per conv
    double vmax = 0.0;
    for (int t = 0; t < 3; ++t)
      for (int ci = 0; ci < 32; ++ci)
        for (int co = 0; co < 32; ++co) {
          const double v = std::fabs((double)w[((size_t)t * 32 + ci) * 32 + co] * scale1[(size_t)q * 32 + co]);
          if (!(v <= 65000.0)) ok = false;            // (also catches NaN)
          vmax = std::max(vmax, v);
        }
    if (vmax != 0.0 && vmax < 0.015625) ok = false;
    if (!ok) break;
    for (int t = 0; t < 3; ++t)
      for (int cc = 0; cc < 2; ++cc)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int co = lane & 31, ci = cc * 16 + (lane >> 5) * 8 + j;
            const float v = (float)((double)w[((size_t)t * 32 + ci) * 32 + co] * scale1[(size_t)q * 32 + co]);
            const float hi = f16_value(v);
            const size_t base = ((((size_t)(q - 1) * 3 + t) * 2 + cc) * 2) * 64 * 8;
            frag[base + (size_t)lane * 8 + j] = f16_bits(hi);
            frag[base + 64 * 8 + (size_t)lane * 8 + j] = f16_bits(v - hi);      // (may be an f16 subnormal: the MFMA honours those)
          }
  }
  // a shortcut saved by layer r is read by exactly the next ADD: saves must not overlap
  if (ok) {
    int pending = -1;
    for (int q = 0; q <= nc; ++q) {
      if (sn->layer[q].add) pending = -1;
      if (sn->layer[q].save) {
        if (pending >= 0) ok = false;
        pending = q;
      }
    }
  }
  // every NMD_FINAL in front of the pool must finish one of the taps (the one most recently written to its slot)
  for (int i = 0; i < pool_op && ok; ++i) {
    if (m->ops[(size_t)i].kind != JG_OP_NMD_FINAL) continue;
    int tap = 0;
    for (int t = 1; t <= sn->n_taps; ++t)
      if (sn->tap_part_slot[t] == m->ops[(size_t)i].arg && sn->tap_conv_op[t] < i) tap = t;
    if (tap == 0 || m->ops[(size_t)i].cout != 32) ok = false;
  }
  if (sn->n_taps > JG_SMALL_MAX_LAYERS) ok = false;
  if (!ok) { delete sn; return JG_OK; }
  sn->n_slots = 1 + sn->n_taps;
  // first-layer table T_t[id] = E[id] . W_t (f64), row `vocab` = zeros (padding), row 0 = zeros when ids mask
  const int k0 = c0.k, vr = m->vocab + 1, cin_pad = (c0.cin + 1) & ~1;
  std::vector<float> lut((size_t)k0 * vr * 32, 0.f);
  const float *emb = weights + c0.b_off, *w0 = weights + c0.w_off;
  for (int t = 0; t < k0; ++t)
    for (int id = (use_mask ? 1 : 0); id < m->vocab; ++id)
      for (int n = 0; n < 32; ++n) {
        double acc = 0.0;
        for (int ci = 0; ci < c0.cin; ++ci)
          acc += (double)emb[(size_t)id * c0.cin + ci] * (double)w0[((size_t)t * cin_pad + ci) * 32 + n];
        lut[((size_t)t * vr + id) * 32 + n] = (float)(acc * scale1[(size_t)n]);
      }
  // every output position reads exactly one row of tap 0 (a codon's, the masked id 0's or the padding row `vocab`):
  // the first affine's shift rides on all of them
  for (int id = 0; id < vr; ++id)
    for (int n = 0; n < 32; ++n) lut[(size_t)id * 32 + n] = (float)((double)lut[(size_t)id * 32 + n] + shift1[(size_t)n]);
  JG_HIP(hipMalloc(reinterpret_cast<void **>(&sn->d_lut), lut.size() * sizeof(float)));
  JG_HIP(hipMemcpy(sn->d_lut, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
  JG_HIP(hipMalloc(reinterpret_cast<void **>(&sn->d_epi), epi.size() * sizeof(float)));
  JG_HIP(hipMemcpy(sn->d_epi, epi.data(), epi.size() * sizeof(float), hipMemcpyHostToDevice));
  JG_HIP(hipMalloc(reinterpret_cast<void **>(&sn->d_wfrag), frag.size() * 2));
  JG_HIP(hipMemcpy(sn->d_wfrag, frag.data(), frag.size() * 2, hipMemcpyHostToDevice));

  sn->valid = true;
  sn->n_conv = nc;
  sn->k0 = k0;
  sn->pad_same0 = c0.padding == JG_PAD_SAME;
  sn->use_mask = use_mask ? 1 : 0;
  sn->pool_kind = pl.arg;
  sn->first_op = 0;
  sn->pool_op = pool_op;
  sn->flops_per_pos0 = 2.0 * k0 * c0.cin * 32;
  sn->flops_per_pos = 2.0 * 3 * 32 * 32 * nc;
  m->small = sn;
  return JG_OK;
}

// exact-f32 conv operands: weights grouped by 8 input channels so that a lane fetches the four
// k-steps of a group with one 16-byte load (see conv_f32_kernel)
// ---- table net (jg_kernels.hip: tab_conv_pool_kernel) ------------------------------------------------------------
// The program matches when its first op is an UNMASKED stride-1 conv on the ids whose stages are [bias] [activation]
// and whose output goes to an unmasked global pool and nowhere else: the strand branch of the nucleotide model
// (conv1d -> relu -> max1d, train_config/nn_config_500bp_dvf.yaml).  Table entry (t, id) = embedding row id times W[t]
// (f64 sums, rounded once): for one-hot input W[t][id - 1] itself, the zero row for id 0.
int jg_prepare_tab(jg_model *m, const float *weights) {
  if (m->ops.size() < 2 || m->id_frames != 1) return JG_OK;      // (rows of one frame: the pool is per row)
  const jg_op &c = m->ops[0], &pl = m->ops[1];
  if (c.kind != JG_OP_CONV || c.in_buf != JG_BUF_IDS || c.in_mask >= 0 || c.in_mask == JG_BUF_IDS || c.out_mask >= 0 ||
      c.stride != 1 || c.n_stages > 2)
    return JG_OK;
  if (pl.kind != JG_OP_POOL || pl.in_buf != c.out_buf || pl.in_mask >= 0 || pl.in_mask == JG_BUF_IDS) return JG_OK;
  int bias_off = -1, act = JG_ACT_NONE, seen = 0;
  for (int q = 0; q < c.n_stages; ++q) {
    const jg_stage &st = c.stages[q];
    if (st.kind == JG_ST_BIAS && q == 0) { bias_off = (int)st.p0; ++seen; }
    else if (st.kind == JG_ST_ACT && q == c.n_stages - 1) { act = st.arg; ++seen; }
  }
  if (seen != c.n_stages) return JG_OK;
  for (size_t i = 2; i < m->ops.size(); ++i) {                    // the conv's output must have no other reader
    const jg_op &o = m->ops[i];
    if (o.in_buf == c.out_buf || o.out_buf == c.out_buf) return JG_OK;
    for (int q = 0; q < o.n_stages; ++q)
      if (o.stages[q].kind == JG_ST_ADD && o.stages[q].arg == c.out_buf) return JG_OK;
  }
  const int cq = (c.cout + 3) / 4;
  const float *w = weights + c.w_off, *emb = weights + c.b_off;
  // positions outside the sequence (SAME padding) add nothing: they select an all-zero table row - row 0 when the
  // embedding's row 0 is zero (one-hot input), else a row appended behind the vocabulary
  bool row0_zero = true;
  for (int ci = 0; ci < c.cin; ++ci) row0_zero &= emb[ci] == 0.f;
  const int V = m->vocab + (row0_zero ? 0 : 1);
  if (V > 255 || cq > 256 || jg_tab_lds_bytes(c.k, V, cq, 64, c.dilation) > 160 * 1024) return JG_OK;
  const int cin_pad = (c.cin + 1) & ~1, cout_pad = (c.cout + 31) / 32 * 32;
  std::vector<float> tab((size_t)c.k * V * cq * 4, 0.f), bias((size_t)cq * 4, 0.f);
  for (int t = 0; t < c.k; ++t)
    for (int id = 0; id < m->vocab; ++id)
      for (int n = 0; n < c.cout; ++n) {
        double acc = 0.0;
        for (int ci = 0; ci < c.cin; ++ci)
          acc += (double)emb[(size_t)id * c.cin + ci] * (double)w[((size_t)t * cin_pad + ci) * cout_pad + n];
        tab[((size_t)t * V + id) * cq * 4 + n] = (float)acc;
      }
  if (bias_off >= 0)
    for (int n = 0; n < c.cout; ++n) bias[(size_t)n] = weights[bias_off + n];
  JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->tab_table), tab.size() * sizeof(float)));
  JG_HIP(hipMemcpy(m->tab_table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->tab_bias), bias.size() * sizeof(float)));
  JG_HIP(hipMemcpy(m->tab_bias, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  bool f16_range = true;                                          // (a weight beyond the f16 range keeps the exact-f32 form)
  for (float v : tab) f16_range &= std::fabs(v) < 32768.f;
  if (row0_zero && f16_range && jg_tab_mfma_supports(c.k, m->vocab, c.cout, c.dilation)) {
    // the same table as MFMA A-operand fragments (jg_tabnet.hip): [32-channel tile][k-step of 4 taps][hi | lo][lane][8]
    const int ks = (c.k + 3) / 4;
    std::vector<uint16_t> frag((size_t)jg_tab_mfma_frag_halves(c.k), 0);
    for (int tile = 0; tile < 16; ++tile)
      for (int st = 0; st < ks; ++st)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int co = tile * 32 + (lane & 31), kk = (lane >> 5) * 8 + j, tap = 4 * st + kk / 4, nuc = kk % 4;
            if (co >= c.cout || tap >= c.k) continue;
            const float v = tab[((size_t)tap * V + (nuc + 1)) * cq * 4 + co];
            const float hi = f16_value(v);
            const size_t base = (((size_t)tile * ks + st) * 2) * 64 * 8;
            frag[base + (size_t)lane * 8 + j] = f16_bits(hi);
            frag[base + 64 * 8 + (size_t)lane * 8 + j] = f16_bits(v - hi);
          }
    std::vector<float> b512(512, 0.f);
    for (int n = 0; n < c.cout; ++n) b512[(size_t)n] = bias[(size_t)n];
    JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->tab_wfrag), frag.size() * sizeof(uint16_t)));
    JG_HIP(hipMemcpy(m->tab_wfrag, frag.data(), frag.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->tab_bias512), b512.size() * sizeof(float)));
    JG_HIP(hipMemcpy(m->tab_bias512, b512.data(), b512.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  m->tab_conv = 0;
  m->tab_pool = 1;
  m->tab_act = act;
  m->tab_cq = cq;
  m->tab_vocab = V;
  m->tab_zero = row0_zero ? 0 : m->vocab;
  return JG_OK;
}

int jg_prepare_f32(jg_model *m, const float *weights) {
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    if (op.kind != JG_OP_CONV) continue;
    const int cin_pad2 = (op.cin + 1) & ~1, cout_pad = (op.cout + 31) / 32 * 32, cin8 = (op.cin + 7) / 8 * 8;
    const float *w = weights + op.w_off;
    std::vector<float> w8((size_t)op.k * (cin8 / 8) * cout_pad * 8, 0.f);
    for (int t = 0; t < op.k; ++t)
      for (int c = 0; c < op.cin; ++c)
        for (int n = 0; n < op.cout; ++n)
          w8[(((size_t)t * (cin8 / 8) + c / 8) * cout_pad + n) * 8 + c % 8] = w[((size_t)t * cin_pad2 + c) * cout_pad + n];
    JG_HIP(hipMalloc(reinterpret_cast<void **>(&m->hprep[i].d_w8), w8.size() * sizeof(float)));
    JG_HIP(hipMemcpy(m->hprep[i].d_w8, w8.data(), w8.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  return JG_OK;
}

// Does op read / write activation slot `buf` as a tensor?  The format pass, the phase-split plan and the residual-block plan
// all go by these two.
bool jg_op_reads(const jg_op &o, int buf) {
  if ((o.kind == JG_OP_CONV || o.kind == JG_OP_ELTWISE || o.kind == JG_OP_MAXPOOL1D || o.kind == JG_OP_FRAMESUM || o.kind == JG_OP_POOL ||
       o.kind == JG_OP_POOLVEC || o.kind == JG_OP_NMD_FINAL || jg_op_is_mixer(o.kind)) && o.in_buf == buf)
    return true;
  if (o.kind == JG_OP_CONV || o.kind == JG_OP_ELTWISE)
    for (int q = 0; q < o.n_stages; ++q)
      if (o.stages[q].kind == JG_ST_ADD && o.stages[q].arg == buf) return true;
  return false;
}

bool jg_op_writes(const jg_op &o, int buf) {
  return (o.kind == JG_OP_CONV || o.kind == JG_OP_ELTWISE || o.kind == JG_OP_MAXPOOL1D || o.kind == JG_OP_FRAMESUM || o.kind == JG_OP_EMBED ||
          jg_op_is_mixer(o.kind)) && o.out_buf == buf;
}

int jg_prepare_f16(jg_model *m, const float *weights) {
  m->hprep.assign(m->ops.size(), ConvHPrep());
  m->pool_fused_by.assign(m->ops.size(), -1);
  m->f16_eligible = true;
  m->f16_reason.clear();
  // Pass A - every conv on its own: can it run on the split-f16 kernel (taps / dilation inside the tiling, a compiled
  // epilogue pattern; 32, 64 or a multiple of 128 output channels - narrow convs on 64- / 32-channel workgroup tiles,
  // wider ones as one launch per 128 channels; stride 2 as the stride-1 conv whose even outputs are kept)?  Ineligible
  // convs (1x1 bypass, other strides or widths) keep the exact-f32 kernel inside an otherwise split-f16 program; pass B
  // below places the layout conversions between them.
  std::string first_reason;
  size_t cur = 0;
  auto fail = [&](const char *why) {
    if (first_reason.empty()) first_reason = why;
    if (m->hprep[cur].why_f32.empty()) m->hprep[cur].why_f32 = why;
  };
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    if (op.kind != JG_OP_CONV) continue;
    cur = i;
    ConvHPrep &hp = m->hprep[i];
    hp.f16_ok = false;
    if ((int)i == m->tab_conv) { fail("runs as the table-net kernel (exact f32, ids to pooled vectors)"); continue; }
    // a 1x1 conv (the bypass of a strided / widening residual block) and a 3-tap conv (ResidualBlock's default kernel
    // size, layers.py:1787) ride the 5-tap kernel: weights in the middle taps, the matrix-core work of the others skipped
    hp.as_k5 = op.k >= 1 && op.k <= 4 && op.in_buf != JG_BUF_IDS;       // (2- and 4-tap convs the same way)
    const int kk = hp.as_k5 ? 5 : op.k, kdil = (hp.as_k5 && op.k == 1) ? 1 : op.dilation;
    if (op.stride != 1 && !(op.stride == 2 && (kk == 5 || kk == 7 || kk == 9) && op.in_buf != JG_BUF_IDS)) { fail("strided conv"); continue; }
    // (a first conv on ids runs as the table variant whatever its tap count, when the table fits LDS)
    static const bool no_lut = jg_exp_env("JG_NO_LUT") != nullptr;
    const bool lut_ok = !no_lut && op.in_buf == JG_BUF_IDS && (op.in_mask == JG_BUF_IDS || op.in_mask < 0) && op.cout <= 128 &&
                        op.stride == 1 && jg_conv_lut_supports(op.k, op.dilation, m->vocab);
    const bool mfma_ok = jg_conv_f16_supports(kk, kdil);
    if (!mfma_ok && !lut_ok) { fail("taps / dilation outside the split-f16 tiling"); continue; }
    const bool narrow = op.cout == 32 || op.cout == 64;
    if (op.cout % 16 != 0 || !(narrow || (op.cout > 64 && op.cout <= 128) || op.cout % 128 == 0)) {
      fail("conv width is not 32, 64, 80..128 or a multiple of 128 channels");
      continue;
    }
    // (the k = 5, 7 and 9 kernels are all built with run-time output geometry - other widths than 128, stride 2; a first
    // conv of up to 128 channels runs as the table variant, which has it too: no table -> 128 channels only, below)
    if (op.in_buf == JG_BUF_IDS && op.cout > 128) { fail("first conv wider than 128 channels"); continue; }
    if (op.in_buf != JG_BUF_IDS && op.cin % 16 != 0) { fail("conv input width is not a multiple of 16"); continue; }
    bool conv_ok = true;
    auto cfail = [&](const char *why) { conv_ok = false; fail(why); };
    const int cin16 = (op.cin + 15) / 16 * 16, cin_pad = (op.cin + 1) & ~1, cout_pad = 128;
    hp.cc_in = cin16 / 16;
    hp.n_half = (op.cout + 127) / 128;
    hp.cw = (narrow && op.in_buf != JG_BUF_IDS) ? op.cout : 128;    // (a first conv runs as the table variant: 128-wide)
    const int cwide = hp.n_half * 128;                                // channels incl. zero padding
    const float *w = weights + op.w_off;   // (k, cin_pad, cout_pad32) f32
    const int cout_pad32 = (op.cout + 31) / 32 * 32;
    float maxabs = 0.f;
    for (int64_t q = 0; q < (int64_t)op.k * cin_pad * cout_pad32; ++q) maxabs = std::max(maxabs, fabsf(w[q]));
    int sexp = 0;
    if (maxabs > 0.f) {
      int e2;
      frexpf(maxabs, &e2);            // maxabs = f * 2^e2, f in [0.5, 1)
      sexp = 3 - e2;                  // scaled max in [4, 8)
    }
    const float wscale = ldexpf(1.f, sexp);
    hp.acc_scale = ldexpf(1.f, -sexp);
    const int kc_total = cin16 / 8;
    const size_t half_items = (size_t)2 * kk * kc_total * cout_pad;       // one 128-channel half: [plane][tap][kc][128]
    const size_t n_items = half_items * hp.n_half;
    hp.wh_half_items = (int64_t)half_items;
    std::vector<uint16_t> wh(n_items * 8, 0);
    for (int t = 0; t < op.k; ++t)
      for (int c = 0; c < op.cin; ++c)
        for (int n = 0; n < op.cout; ++n) {
          const float v = w[((size_t)t * cin_pad + c) * cout_pad32 + n] * wscale;
          const float hi = f16_value(v);
          const size_t base = (size_t)(n / 128) * half_items;
          const int tk = hp.as_k5 ? std::max(1, (5 - op.k) / 2) + t : t;   // (a 1x1 / 3-tap conv's taps sit in the middle of five)
          const size_t item = base + (((size_t)0 * kk + tk) * kc_total + c / 8) * cout_pad + n % 128;
          const size_t item_lo = base + (((size_t)1 * kk + tk) * kc_total + c / 8) * cout_pad + n % 128;
          wh[item * 8 + c % 8] = f16_bits(hi);
          wh[item_lo * 8 + c % 8] = f16_bits(v - hi);
        }
    JG_HIP(hipMalloc(reinterpret_cast<void **>(&hp.d_wh), n_items * 16));
    JG_HIP(hipMemcpy(hp.d_wh, wh.data(), n_items * 16, hipMemcpyHostToDevice));
    if (op.in_buf == JG_BUF_IDS) {
      const float *emb = weights + op.b_off;   // (vocab, cin)
      const size_t e_items = (size_t)m->vocab * hp.cc_in * 4;
      std::vector<uint16_t> eh(e_items * 8, 0);
      for (int id = 0; id < m->vocab; ++id)
        for (int c = 0; c < op.cin; ++c) {
          const float v = emb[(size_t)id * op.cin + c];
          const float hi = f16_value(v);
          if (!(fabsf(v) <= 65000.f)) cfail("embedding value outside the f16 range");
          const int cc = c / 16, hh = (c % 16) / 8, j = c % 8;
          eh[(((size_t)id * hp.cc_in + cc) * 4 + 0 * 2 + hh) * 8 + j] = f16_bits(hi);
          eh[(((size_t)id * hp.cc_in + cc) * 4 + 1 * 2 + hh) * 8 + j] = f16_bits(v - hi);
        }
      JG_HIP(hipMalloc(reinterpret_cast<void **>(&hp.d_embh), e_items * 16));
      JG_HIP(hipMemcpy(hp.d_embh, eh.data(), e_items * 16, hipMemcpyHostToDevice));
    }
    // compact epilogue: fold acc un-scale, bias and batch-norm chains into per-channel affines
    {
      std::vector<float> tab;                       // [n_epi_rows][2][cwide]; uploaded as [half][n_epi_rows][2][128]
      std::vector<double> sc(cwide, (double)hp.acc_scale), sh(cwide, 0.0);
      bool pending = true;                          // an affine (the un-scale) is always pending first
      hp.n_hst = 0;
      hp.n_epi_rows = 0;
      auto flush = [&]() {
        if (!pending) return;
        HStageArg h{JG_HST_AFFINE, 0, 0.f, hp.n_epi_rows++};
        hp.hst[hp.n_hst++] = h;
        for (int n = 0; n < cwide; ++n) tab.push_back((float)sc[n]);
        for (int n = 0; n < cwide; ++n) tab.push_back((float)sh[n]);
        std::fill(sc.begin(), sc.end(), 1.0);
        std::fill(sh.begin(), sh.end(), 0.0);
        pending = false;
      };
      for (int q = 0; q < op.n_stages && conv_ok; ++q) {
        const jg_stage &st = op.stages[q];
        auto vecp = [&](int64_t off) { return weights + off; };
        if (st.kind == JG_ST_BIAS) {
          for (int n = 0; n < op.cout; ++n) sh[n] += (double)vecp(st.p0)[n];
          pending = true;
          continue;
        }
        if (st.kind == JG_ST_BN) {   // g*((x-mu)*is)+b on top of x = v*sc+sh
          for (int n = 0; n < op.cout; ++n) {
            const double mu = vecp(st.p0)[n], is = vecp(st.p1)[n], g = vecp(st.p2)[n], b = vecp(st.p3)[n];
            sc[n] = sc[n] * is * g;
            sh[n] = (sh[n] - mu) * is * g + b;
          }
          pending = true;
          continue;
        }
        flush();
        if (hp.n_hst >= JG_MAX_STAGES) { cfail("epilogue too long"); break; }
        HStageArg h{0, st.arg, st.f0, 0};
        switch (st.kind) {
          case JG_ST_DYT:
            h.kind = JG_HST_DYT;
            h.pad_ = hp.n_epi_rows++;
            for (int n = 0; n < cwide; ++n) tab.push_back(n < op.cout ? vecp(st.p2)[n] : 0.f);
            for (int n = 0; n < cwide; ++n) tab.push_back(n < op.cout ? vecp(st.p3)[n] : 0.f);
            break;
          case JG_ST_ADD: h.kind = JG_HST_ADD; hp.add_slot = st.arg; break;
          case JG_ST_ACT:
            h.kind = JG_HST_ACT;
            break;
          case JG_ST_NMD:
            h.kind = JG_HST_NMD;
            if (hp.nmd_slot < 0) hp.nmd_slot = st.arg;
            else if (hp.nmd_slot2 < 0) hp.nmd_slot2 = st.arg;
            else cfail("more than two NMD taps in one conv");
            break;
          case JG_ST_MASKMUL: h.kind = JG_HST_MASKMUL; break;
          default: cfail("epilogue stage not supported by the split-f16 kernel"); break;
        }
        hp.hst[hp.n_hst++] = h;
      }
      if (conv_ok) {
        if (pending && hp.n_hst >= JG_MAX_STAGES) cfail("epilogue too long");
        else flush();
      }
      if (hp.n_epi_rows > JG_EPI_ROWS) cfail("more norm stages than the split-f16 epilogue table holds");
      // match the stage list against the compiled pattern
      //   affine [nmd] [norm1] [add] [gelu] [nmd] [norm2] [gelu]
      {
        unsigned ep = 0;
        int q = 0;
        const int n = hp.n_hst;
        auto is = [&](int kind) { return q < n && hp.hst[q].kind == kind; };
        bool ok = is(JG_HST_AFFINE);
        if (ok) {
          ++q;
          if (is(JG_HST_NMD)) { ep |= JG_EP_NMD1; ++q; }
          if (is(JG_HST_AFFINE)) { ep |= JG_EP_NORM1_AFF; ++q; }
          else if (is(JG_HST_DYT)) { ep |= JG_EP_NORM1_DYT; hp.alpha1 = hp.hst[q].f0; hp.dytmask1 = hp.hst[q].arg; ++q; }
          if (is(JG_HST_ADD)) { ep |= JG_EP_ADD; ++q; }
          int gelu_kind = 0;   // all activation stages of a compiled pattern share one kind
          auto is_gelu = [&]() {
            if (!is(JG_HST_ACT)) return false;
            const int k = hp.hst[q].arg;
            if (k != JG_ACT_GELU_TANH && k != JG_ACT_GELU_ERF && k != JG_ACT_RELU) return false;
            if (gelu_kind != 0 && gelu_kind != k) return false;
            gelu_kind = k;
            return true;
          };
          if (is_gelu()) { ep |= JG_EP_ACT1; ++q; }
          if (is(JG_HST_NMD)) { ep |= JG_EP_NMD2; ++q; }
          if (is(JG_HST_AFFINE)) { ep |= JG_EP_NORM2_AFF; ++q; }
          else if (is(JG_HST_DYT)) { ep |= JG_EP_NORM2_DYT; hp.alpha2 = hp.hst[q].f0; hp.dytmask2 = hp.hst[q].arg; ++q; }
          if (is_gelu()) { ep |= JG_EP_ACT2; ++q; }
          ok = q == n;
          hp.act_kind = gelu_kind != 0 ? gelu_kind : JG_ACT_GELU_TANH;
        }
        if (ok && (ep & (JG_EP_NORM1_DYT | JG_EP_NORM2_DYT)) && (ep & (JG_EP_ACT1 | JG_EP_ACT2)) &&
            hp.act_kind != JG_ACT_GELU_TANH)
          ok = false;               // the DyT patterns are compiled for the tanh-GELU only
        hp.ep = ok ? ep : JG_EP_GENERIC;
        hp.ep_rt = 0;
        // a canonical stage list without an instantiation of its own (incl. two NMD taps in one conv): the run-time-flag
        // epilogue - tanh-GELU stage lists only (it carries every stage kind at once; the erf / ReLU forms beside them spill)
        const bool narrow_geo = op.in_buf != JG_BUF_IDS && (op.cout != 128 || op.stride != 1 || hp.as_k5);
        if (ok && hp.act_kind == JG_ACT_GELU_TANH && !(ep & JG_EP_ADD && op.in_buf == JG_BUF_IDS) &&
            (!jg_conv_f16_has_pattern(ep, op.in_buf == JG_BUF_IDS) || (narrow_geo && !jg_conv_f16_has_narrow_pattern(ep)) ||
             ((ep & JG_EP_NMD1) && (ep & JG_EP_NMD2)))) {
          hp.ep_rt = ep;
          hp.ep = JG_EP_RUNTIME;
        }
        if (hp.ep != JG_EP_RUNTIME && hp.nmd_slot2 >= 0) ok = false, hp.ep = JG_EP_GENERIC;   // two taps need the second accumulator
        // Only compiled stage patterns run on the split-f16 path: the interpreted epilogue was measured
        // 12x slower than the compiled ones (and 3x slower than the exact-f32 kernels), so anything else
        // stays on the exact-f32 path.
        if (conv_ok && !jg_conv_f16_has_pattern(hp.ep, op.in_buf == JG_BUF_IDS)) {
          cfail("a conv's stage list is not one of the compiled split-f16 epilogue patterns");
        }
        if (conv_ok && op.in_buf != JG_BUF_IDS && (op.cout != 128 || op.stride != 1 || hp.as_k5) && !jg_conv_f16_has_narrow_pattern(hp.ep))
          cfail("the stage list of a conv of other than 128 channels / stride 1 is not one of the patterns compiled for it");
        if (conv_ok && op.stride == 2 && ((hp.ep == JG_EP_RUNTIME ? hp.ep_rt : hp.ep) & (JG_EP_ADD | JG_EP_NMD1 | JG_EP_NMD2)))
          cfail("strided conv with a shortcut or an NMD tap in its epilogue");
      }
      if (conv_ok) {
        std::vector<float> th(tab.size());                 // [half][row][2][128]
        const int nr = hp.n_epi_rows;
        for (int hf = 0; hf < hp.n_half; ++hf)
          for (int r = 0; r < nr * 2; ++r)
            for (int n = 0; n < 128; ++n) th[((size_t)hf * nr * 2 + r) * 128 + n] = tab[(size_t)r * cwide + hf * 128 + n];
        JG_HIP(hipMalloc(reinterpret_cast<void **>(&hp.d_epi), th.size() * sizeof(float)));
        JG_HIP(hipMemcpy(hp.d_epi, th.data(), th.size() * sizeof(float), hipMemcpyHostToDevice));
      }
      // first layer on ids: the conv is a sum of k table rows T_t[id] = E[id] . W_t (f64 on the
      // host); the kernel's table variant then needs no matrix cores and no acc un-scale
      if (conv_ok && lut_ok) {
        const float *emb = weights + op.b_off;   // (vocab, cin)
        const int vr = m->vocab + 1;             // + the all-zero padding row
        std::vector<float> lut((size_t)2 * op.k * vr * 64, 0.f);
        for (int t = 0; t < op.k; ++t)
          for (int id = (op.in_mask == JG_BUF_IDS ? 1 : 0); id < m->vocab; ++id)   // id 0 is masked: zero row
            for (int n = 0; n < op.cout; ++n) {
              double acc = 0.0;
              for (int c = 0; c < op.cin; ++c)
                acc += (double)emb[(size_t)id * op.cin + c] * (double)w[((size_t)t * cin_pad + c) * cout_pad32 + n];
              lut[(((size_t)(n >> 6) * op.k + t) * vr + id) * 64 + (n & 63)] = (float)acc;
            }
        std::vector<float> tab_lut(tab);
        for (int n = 0; n < 128; ++n) tab_lut[n] = (float)((double)tab[n] / (double)hp.acc_scale);   // row 0 scale
        JG_HIP(hipMalloc(reinterpret_cast<void **>(&hp.d_lut), lut.size() * sizeof(float)));
        JG_HIP(hipMemcpy(hp.d_lut, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
        JG_HIP(hipMalloc(reinterpret_cast<void **>(&hp.d_epi_lut), tab_lut.size() * sizeof(float)));
        JG_HIP(hipMemcpy(hp.d_epi_lut, tab_lut.data(), tab_lut.size() * sizeof(float), hipMemcpyHostToDevice));
      }
      if (conv_ok && op.in_buf == JG_BUF_IDS && hp.d_lut == nullptr && (op.cout != 128 || !mfma_ok))
        cfail("first conv without the table variant is not a 128-channel 5- / 7- / 9-tap conv");
    }
    hp.f16_ok = conv_ok;
  }
  // Pass B - tensor formats.  Walk the program with the format of every activation slot (f32 rows or F16S items):
  // split-f16 convs read and write F16S (f32 when the next reader needs it, or no tensor at all when only a max pool
  // reads it), everything else works on f32; where a reader meets the other format, a layout conversion is queued in
  // front of it (run_chunk converts into a scratch tensor and swaps the slot's pointer).
  int n_ok = 0, n_conv = 0;
  for (size_t i = 0; i < m->ops.size(); ++i)
    if (m->ops[i].kind == JG_OP_CONV) { ++n_conv; n_ok += m->hprep[i].f16_ok ? 1 : 0; }
  if (n_ok == 0) {
    m->f16_eligible = false;
    m->f16_reason = first_reason.empty() ? "program has no convolution" : first_reason;
    return JG_OK;
  }
  m->f16_mixed = n_ok < n_conv;
  bool is_f32[JG_MAX_BUFS] = {};
  auto wants_f16s = [&](size_t j, int buf) {          // does op j read `buf` as an F16S tensor?
    const jg_op &o = m->ops[j];
    if (o.kind == JG_OP_MAXPOOL1D && o.in_buf == buf) return true;
    if (o.kind != JG_OP_CONV || !m->hprep[j].f16_ok) return false;
    if (o.in_buf == buf) return true;
    for (int q = 0; q < o.n_stages; ++q)
      if (o.stages[q].kind == JG_ST_ADD && o.stages[q].arg == buf) return true;
    return false;
  };
  // (NMD_FINAL only takes the slot's shape: no format is asked of it)
  auto reads = [&](size_t j, int buf) { return m->ops[j].kind != JG_OP_NMD_FINAL && jg_op_reads(m->ops[j], buf); };
  bool cvt_overflow = false;
  auto need = [&](size_t i, int buf, bool want_f32) {   // queue a conversion in front of op i if the slot is in the other format
    if (buf < 0 || is_f32[buf] == want_f32) return;
    ConvHPrep &hp = m->hprep[i];
    if (hp.n_cvt >= 3) {           // table full: the op would read a tensor in the wrong layout - give the fast path up instead
      cvt_overflow = true;
      return;
    }
    hp.cvt_slot[hp.n_cvt] = buf;
    hp.cvt_to_f32[hp.n_cvt] = want_f32;
    ++hp.n_cvt;
    is_f32[buf] = want_f32;
    m->needs_cvt = true;
  };
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    ConvHPrep &hp = m->hprep[i];
    switch (op.kind) {
      case JG_OP_CONV: {
        const bool f16 = hp.f16_ok;
        need(i, op.in_buf, !f16);
        for (int q = 0; q < op.n_stages; ++q)
          if (op.stages[q].kind == JG_ST_ADD) need(i, op.stages[q].arg, !f16);
        if (!f16) { is_f32[op.out_buf] = true; break; }
        // output format: what the first reader wants
        bool first_f16s = false, any_reader = false;
        for (size_t j = i + 1; j < m->ops.size(); ++j) {
          if (reads(j, op.out_buf)) { first_f16s = wants_f16s(j, op.out_buf); any_reader = true; break; }
          if (jg_op_writes(m->ops[j], op.out_buf)) break;
        }
        hp.out_f16s = any_reader && first_f16s;
        is_f32[op.out_buf] = !hp.out_f16s;
        if (!hp.out_f16s && jg_exp_env("JG_NO_POOL_FUSE") == nullptr) {
          // the only reader of the f32 output is a masked global max pool over the conv's own output mask:
          // reduce in the epilogue instead of storing 4 B per element and reading it back
          int readers = 0, pool_idx = -1;
          for (size_t j = i + 1; j < m->ops.size(); ++j) {
            const jg_op &o = m->ops[j];
            if (reads(j, op.out_buf)) {
              ++readers;
              if (o.kind == JG_OP_POOL && o.arg == JG_POOL_MAX && o.in_mask == op.out_mask) pool_idx = (int)j;
              else pool_idx = -2;
            }
            if (jg_op_writes(m->ops[j], op.out_buf)) break;
          }
          if (readers == 1 && pool_idx >= 0) {
            hp.pool_op = pool_idx;
            m->pool_fused_by[(size_t)pool_idx] = (int)i;
          }
        }
      } break;
      case JG_OP_EMBED:
        is_f32[op.out_buf] = true;                      // the lookup writes f32 rows: the first conv converts if it wants F16S
        break;
      case JG_OP_ELTWISE:
        need(i, op.in_buf, true);
        for (int q = 0; q < op.n_stages; ++q)
          if (op.stages[q].kind == JG_ST_ADD) need(i, op.stages[q].arg, true);
        is_f32[op.out_buf] = true;
        break;
      case JG_OP_MAXPOOL1D:
        hp.pool_f16s = op.in_buf >= 0 && !is_f32[op.in_buf];
        is_f32[op.out_buf] = !hp.pool_f16s;
        break;
      case JG_OP_FRAMESUM:
        need(i, op.in_buf, true);
        is_f32[op.out_buf] = true;
        break;
      case JG_OP_POOL:
        if (m->pool_fused_by[i] < 0) need(i, op.in_buf, true);
        break;
      case JG_OP_POOLVEC:                               // f32 rows, never fused into its producer's epilogue
        need(i, op.in_buf, true);
        break;
      default:
        if (!jg_op_is_mixer(op.kind)) break;            // f32 rows in and out: an F16S producer is converted in front of it
        need(i, op.in_buf, true);
        is_f32[op.out_buf] = true;
        break;
    }
  }
  if (cvt_overflow) {
    m->f16_eligible = false;
    m->f16_mixed = false;
    m->f16_reason = "an op needs more than 3 layout conversions in front of it (mixed split-f16 / f32 program)";
    for (ConvHPrep &hp : m->hprep) { hp.f16_ok = false; hp.n_cvt = 0; hp.pool_op = -1; }
    std::fill(m->pool_fused_by.begin(), m->pool_fused_by.end(), -1);
  }
  return JG_OK;
}

// Pass C - stride-2 convs without dropped work.  A strided residual block (layers.py:1882-1915: conv1 of 5 taps and the
// 1x1 bypass, both stride 2, both reading the block's input) is evaluated by the split-f16 kernel at stride 1 with every
// second output dropped.  When ALL readers of a tensor are such convs and a split-f16 conv writes it, the writer stores it
// phase-split instead (ConvHArgs::psplit: even positions in the first cin channels, odd ones in the next cin, (L + 1) / 2
// positions, mask-multiplied) and the readers run at stride 1: the 5-tap conv as a 3-tap conv over 2 x cin channels -
//   y[m] = sum_t w_t x[2m + t - pl]  =  sum over q = t - pl of  w_t . phase(q mod 2)[m + floor(q / 2)]
// (pl = TF's SAME left pad: 2 for an odd input length, 1 for an even one - two weight arrangements) - the 1x1 conv on the
// even phase alone.  Same sums in another order of the taps: results agree to f32 rounding, no output is computed twice.
int jg_plan_phase_split(jg_model *m, const float *weights) {
  if (!m->f16_eligible) return JG_OK;
  static const bool off = jg_exp_env("JG_NO_PSPLIT") != nullptr;
  if (off) return JG_OK;
  const size_t n = m->ops.size();
  for (size_t p = 0; p < n; ++p) {
    const jg_op &po = m->ops[p];
    ConvHPrep &pp = m->hprep[p];
    if (po.kind != JG_OP_CONV || !pp.f16_ok || !pp.out_f16s || pp.pool_op >= 0 || po.stride != 1 || po.out_buf < 0 ||
        po.cout % 16 != 0 || (int)p == m->tab_conv || po.in_buf == JG_BUF_IDS ||
        !jg_conv_f16_has_narrow_pattern(pp.ep))           // (the store is built into the run-time-geometry tiles)
      continue;
    std::vector<size_t> readers;
    bool ok = true, mask_rewritten = false;
    for (size_t j = p + 1; j < n && ok; ++j) {
      const jg_op &o = m->ops[j];
      if (jg_op_reads(m->ops[j], po.out_buf)) {
        const ConvHPrep &hr = m->hprep[j];
        const bool conv_reader = o.kind == JG_OP_CONV && o.in_buf == po.out_buf && hr.f16_ok && o.stride == 2 &&
                                 o.padding == JG_PAD_SAME && o.cin == po.cout && o.in_mask == po.out_mask &&
                                 ((o.k == 5 && o.dilation == 1) || o.k == 1);
        bool adds_it = false;
        for (int q = 0; q < o.n_stages; ++q) adds_it |= o.stages[q].kind == JG_ST_ADD && o.stages[q].arg == po.out_buf;
        bool cvt_here = false;
        for (int q = 0; q < hr.n_cvt; ++q) cvt_here |= hr.cvt_slot[q] == po.out_buf;
        // (the mask the writer multiplies by must still be the reader's input mask when it runs)
        if (!conv_reader || adds_it || cvt_here || mask_rewritten) ok = false;
        else readers.push_back(j);
      }
      if ((o.kind == JG_OP_MASK || o.kind == JG_OP_MSMASK) && po.out_mask >= 0 && o.out_mask == po.out_mask) mask_rewritten = true;
      if (jg_op_writes(m->ops[j], po.out_buf)) break;
    }
    if (!ok || readers.empty()) continue;
    // weights of the 5-tap readers, re-arranged for both parities of the input length
    bool built = true;
    for (size_t j : readers) {
      const jg_op &o = m->ops[j];
      ConvHPrep &hr = m->hprep[j];
      if (o.k != 5) continue;
      const int cin = o.cin, cin2 = 2 * cin, cout_pad32 = (o.cout + 31) / 32 * 32, cin_pad = (cin + 1) & ~1;
      const float *w = weights + o.w_off;                  // (5, cin_pad, cout_pad32)
      const float wscale = 1.0f / hr.acc_scale;            // the conv's own power-of-two scale (the epilogue table undoes it)
      const int kk = 5, kc_total = cin2 / 8, cout_pad = 128;
      const size_t half_items = (size_t)2 * kk * kc_total * cout_pad, n_items = half_items * hr.n_half;
      hr.ps_half_items = (int64_t)half_items;
      for (int par = 0; par < 2; ++par) {                   // par = input length & 1
        const int pl = par ? 2 : 1;
        std::vector<uint16_t> wh(n_items * 8, 0);
        for (int t = 0; t < 5; ++t) {
          const int q = t - pl, ph = ((q % 2) + 2) % 2, off3 = (q - ph) / 2 + 1;     // phase, tap of the 3-tap conv (0 .. 2)
          const int tk = 1 + off3;                                                   // ... in the middle of the kernel's five
          for (int c = 0; c < cin; ++c)
            for (int nn = 0; nn < o.cout; ++nn) {
              const float v = w[((size_t)t * cin_pad + c) * cout_pad32 + nn] * wscale;
              const float hi = f16_value(v);
              const int c2 = ph * cin + c;
              const size_t base = (size_t)(nn / 128) * half_items;
              const size_t item = base + (((size_t)0 * kk + tk) * kc_total + c2 / 8) * cout_pad + nn % 128;
              const size_t item_lo = base + (((size_t)1 * kk + tk) * kc_total + c2 / 8) * cout_pad + nn % 128;
              wh[item * 8 + c2 % 8] = f16_bits(hi);
              wh[item_lo * 8 + c2 % 8] = f16_bits(v - hi);
            }
        }
        if (hipMalloc(reinterpret_cast<void **>(&hr.d_wh_ps[par]), n_items * 16) != hipSuccess ||
            hipMemcpy(hr.d_wh_ps[par], wh.data(), n_items * 16, hipMemcpyHostToDevice) != hipSuccess) {
          built = false;
          break;
        }
      }
      if (!built) break;
    }
    if (!built) {
      (void)hipGetLastError();
      for (size_t j : readers)
        for (int par = 0; par < 2; ++par)
          if (m->hprep[j].d_wh_ps[par]) { (void)hipFree(m->hprep[j].d_wh_ps[par]); m->hprep[j].d_wh_ps[par] = nullptr; }
      continue;
    }
    pp.ps_store = true;
    for (size_t j : readers) m->hprep[j].ps_read = m->ops[j].k == 5 ? 1 : 2;
  }
  return JG_OK;
}

// Pass D - whole narrow residual blocks as one launch (jg_resblock.hip).  conv1 [bias, norm, GELU] and conv2 [bias, norm,
// + block input, GELU] of a stride-1 block without bypass (layers.py:1882-1915), 32 channels, five taps, one dilation: the
// intermediate tensor lives in LDS only.  conv1's op is skipped at run time, conv2's launch computes both; the mask ops
// between them run as before (the kernel reads conv2's input mask from their output).
int jg_plan_resblocks(jg_model *m, const float *weights) {
  if (!m->f16_eligible) return JG_OK;
  static const bool off = jg_exp_env("JG_NO_RESBLOCK") != nullptr;
  if (off) return JG_OK;
  const size_t n = m->ops.size();
  // bias / batch-norm stages in front of the first other stage, folded with the weights' un-scale (as prepare_f16 does)
  auto fold = [&](const jg_op &op, float acc_scale, float *sc, float *sh) {
    std::vector<double> s((size_t)op.cout, (double)acc_scale), t((size_t)op.cout, 0.0);
    for (int q = 0; q < op.n_stages; ++q) {
      const jg_stage &st = op.stages[q];
      if (st.kind == JG_ST_BIAS) {
        for (int c = 0; c < op.cout; ++c) t[(size_t)c] += (double)weights[st.p0 + c];
      } else if (st.kind == JG_ST_BN) {
        for (int c = 0; c < op.cout; ++c) {
          const double mu = weights[st.p0 + c], is = weights[st.p1 + c], g = weights[st.p2 + c], b = weights[st.p3 + c];
          s[(size_t)c] = s[(size_t)c] * is * g;
          t[(size_t)c] = (t[(size_t)c] - mu) * is * g + b;
        }
      } else {
        break;
      }
    }
    for (int c = 0; c < op.cout; ++c) { sc[c] = (float)s[(size_t)c]; sh[c] = (float)t[(size_t)c]; }
  };
  for (size_t ia = 0; ia < n; ++ia) {
    const jg_op &A = m->ops[ia];
    ConvHPrep &ha = m->hprep[ia];
    if (A.kind != JG_OP_CONV || !ha.f16_ok || ha.rb_second >= 0 || ha.rb_first >= 0 || A.in_buf < 0 || A.stride != 1 ||
        A.padding != JG_PAD_SAME || A.cin != A.cout || !(jg_resblock_supports(A.cout, A.k, A.dilation) || jg_resblock64_supports(A.cout, A.k, A.dilation)) || !ha.out_f16s ||
        ha.ep != JG_EP_ACT1 || ha.act_kind != JG_ACT_GELU_TANH || ha.pool_op >= 0 || ha.ps_store || ha.ps_read != 0 ||
        ha.n_cvt != 0 || (int)ia == m->tab_conv)
      continue;
    // the only reader of conv1's output: conv2, before anything overwrites it (mask ops may sit in between)
    size_t ib = n;
    bool ok = true;
    for (size_t j = ia + 1; j < n; ++j) {
      if (jg_op_reads(m->ops[j], A.out_buf)) {
        if (ib == n && m->ops[j].kind == JG_OP_CONV && m->ops[j].in_buf == A.out_buf) ib = j;
        else ok = false;
      }
      if (jg_op_writes(m->ops[j], A.out_buf) && j != ib) break;
      if (jg_op_writes(m->ops[j], A.out_buf) && j == ib) { ok = false; break; }       // (in place: not a residual block)
    }
    if (!ok || ib == n) continue;
    for (size_t j = ia + 1; j < ib && ok; ++j)                               // nothing but mask ops between the two
      ok = m->ops[j].kind == JG_OP_MASK && m->ops[j].out_mask != A.in_mask && m->ops[j].out_mask != A.out_mask;
    const jg_op &B = m->ops[ib];
    ConvHPrep &hb = m->hprep[ib];
    if (!ok || !hb.f16_ok || B.stride != 1 || B.padding != JG_PAD_SAME || B.k != A.k || B.dilation != A.dilation ||
        B.cin != A.cout || B.cout != A.cout || B.in_mask != A.out_mask || !hb.out_f16s ||
        hb.ep != (JG_EP_ADD | JG_EP_ACT1) || hb.act_kind != JG_ACT_GELU_TANH || hb.add_slot != A.in_buf ||
        B.out_buf == A.in_buf || B.out_buf == A.out_buf || hb.pool_op >= 0 || hb.ps_read != 0 || hb.n_cvt != 0 ||
        hb.nmd_slot >= 0 || ha.nmd_slot >= 0)
      continue;
    // weight fragments [conv][tap][chunk][plane][32-channel output tile][lane][8 halfs]: lane = (cin group of 8) x (output
    // channel of the tile)
    const int C = A.cout, K = A.k, cc_n = C / 16, ct_n = C / 32;
    std::vector<uint16_t> frag((size_t)2 * K * cc_n * 2 * ct_n * 64 * 8, 0);
    std::vector<float> epi((size_t)4 * C, 0.f);
    bool range_ok = true;
    for (int c = 0; c < 2; ++c) {
      const jg_op &op = c == 0 ? A : B;
      const ConvHPrep &hp = c == 0 ? ha : hb;
      const float *w = weights + op.w_off;                 // (k, cin_pad, cout_pad32)
      const int cin_pad = (op.cin + 1) & ~1, cout_pad32 = (op.cout + 31) / 32 * 32;
      const float wscale = 1.0f / hp.acc_scale;
      for (int t = 0; t < K; ++t)
        for (int cc = 0; cc < cc_n; ++cc)
          for (int ct = 0; ct < ct_n; ++ct)
            for (int lane = 0; lane < 64; ++lane)
              for (int j = 0; j < 8; ++j) {
                const int co = ct * 32 + (lane & 31), ci = cc * 16 + (lane >> 5) * 8 + j;
                const float v = w[((size_t)t * cin_pad + ci) * cout_pad32 + co] * wscale;
                const float hi = f16_value(v);
                if (!(fabsf(v) <= 65000.f)) range_ok = false;
                const size_t base = ((((size_t)c * K + t) * cc_n + cc) * 2) * ct_n * 64 * 8;
                frag[base + ((size_t)ct * 64 + lane) * 8 + j] = f16_bits(hi);
                frag[base + ((size_t)(ct_n + ct) * 64 + lane) * 8 + j] = f16_bits(v - hi);
              }
      fold(op, hp.acc_scale, epi.data() + (size_t)c * 2 * C, epi.data() + (size_t)c * 2 * C + C);
    }
    if (!range_ok) continue;
    if (hipMalloc(reinterpret_cast<void **>(&hb.d_rb_wfrag), frag.size() * 2) != hipSuccess ||
        hipMemcpy(hb.d_rb_wfrag, frag.data(), frag.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&hb.d_rb_epi), epi.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(hb.d_rb_epi, epi.data(), epi.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      if (hb.d_rb_wfrag) { (void)hipFree(hb.d_rb_wfrag); hb.d_rb_wfrag = nullptr; }
      if (hb.d_rb_epi) { (void)hipFree(hb.d_rb_epi); hb.d_rb_epi = nullptr; }
      continue;
    }
    ha.rb_second = (int)ib;
    hb.rb_first = (int)ia;
  }
  return JG_OK;
}
