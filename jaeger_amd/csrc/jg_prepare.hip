// Model preparation (host): which kernels the op program matches, and every operand those kernels read.  The passes, in
// the order jg_model_create (jg_model.hip) calls them - what they decide is read back through jg_place_op (jg_run.hip):
//   jg_prepare_tab        the table net (first conv + pool as one kernel)
//   jg_prepare_f16        every conv on its own on the split-f16 kernels (geometry, weights, epilogue, pattern, first-layer
//                         table), then jg_plan_formats: tensor formats, layout conversions, fused max pools
//   jg_plan_phase_split   stride-2 convs without dropped work
//   jg_plan_resblocks     whole narrow residual blocks as one launch
//   jg_prepare_f32        exact-f32 conv weights
//   jg_prepare_small      the fused small-window network
// They share one definition each of: the upload (which lists the operand for jg_operand_digest), the bias / batch-norm fold,
// the first-layer dot product, the hi / lo split with the item-layout and lane-fragment writers, and the walk over the
// readers of a slot.
#include "jg_host.h"

// ---- upload, and the digest of what was uploaded ----------------------------------------------------------------------
// owners of the operands that belong to no conv op (a conv's are keyed by its op index)
static const uint64_t KEY_TABNET = 0x7461626e6574ull, KEY_SMALL = 0x736d616c6cull;

// A host vector as a device buffer of its own.  Every operand goes through here and is listed with its owner's key.
template <typename T, typename D>
static hipError_t upload(jg_model *m, uint64_t key, const std::vector<T> &v, D **dst) {
  const size_t bytes = v.size() * sizeof(T);
  hipError_t err = hipMalloc(reinterpret_cast<void **>(dst), bytes);
  if (err == hipSuccess) err = hipMemcpy(*dst, v.data(), bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess) m->operands.push_back({*dst, bytes, key});
  return err;
}
// ... and a plan that gives up takes its buffers back
template <typename D>
static void release(jg_model *m, D **p) {
  if (*p == nullptr) return;
  (void)hipFree(*p);
  for (size_t q = m->operands.size(); q-- > 0;)
    if (m->operands[q].dev == *p) m->operands.erase(m->operands.begin() + (long)q);
  *p = nullptr;
}

// JG_MSTAT_OPERAND_DIGEST: the sum mod 2^64 (so the order of the uploads does not matter) of one 64-bit FNV-1a hash per
// operand - of its owner's key (eight bytes, low first), then of its bytes as they sit on the device.  Computed when asked
// for: hashing at upload time was measured to add 30 ms (a half) to the creation of the pyramid model.
// tests/test_gpu_operand_digest.py pins it.
int64_t jg_operand_digest(const jg_model *m) {
  uint64_t sum = 0;
  std::vector<unsigned char> host;
  for (const jg_model::Operand &o : m->operands) {
    host.resize(o.bytes);
    if (o.bytes != 0 && hipMemcpy(host.data(), o.dev, o.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    uint64_t h = 0xcbf29ce484222325ull;
    for (int b = 0; b < 8; ++b) h = (h ^ ((o.key >> (8 * b)) & 0xff)) * 0x100000001b3ull;
    for (unsigned char c : host) h = (h ^ c) * 0x100000001b3ull;
    sum += h;
  }
  return (int64_t)sum;
}

// ---- bias / batch-norm fold ------------------------------------------------------------------------------------------
// Folds the run of JG_ST_BIAS / JG_ST_BN stages of `op` that starts at stage q into x * sc + sh (f64, the first n
// channels; the caller sets the start values) and returns the first stage it did not consume.
static int fold_affine(const jg_op &op, int q, const float *weights, int n, double *sc, double *sh) {
  for (; q < op.n_stages; ++q) {
    const jg_stage &st = op.stages[q];
    if (st.kind == JG_ST_BIAS) {
      for (int c = 0; c < n; ++c) sh[c] += (double)weights[st.p0 + c];
    } else if (st.kind == JG_ST_BN) {   // g*((x-mu)*is)+b on top of x = v*sc+sh
      for (int c = 0; c < n; ++c) {
        const double mu = weights[st.p0 + c], is = weights[st.p1 + c], g = weights[st.p2 + c], b = weights[st.p3 + c];
        sc[c] = sc[c] * is * g;
        sh[c] = (sh[c] - mu) * is * g + b;
      }
    } else break;
  }
  return q;
}

// ---- first-layer table entry -----------------------------------------------------------------------------------------
// (E[id] . W_t)[n] in f64: emb (vocab, cin), w (k, cin_pad, cout_pad).  The three table builders round it themselves.
static double first_layer_dot(const float *emb, const float *w, int id, int t, int n, int cin, int cin_pad, int cout_pad) {
  double acc = 0.0;
  for (int c = 0; c < cin; ++c) acc += (double)emb[(size_t)id * cin + c] * (double)w[((size_t)t * cin_pad + c) * cout_pad + n];
  return acc;
}

// ---- split-f16 packing: see jg_conv_f16.hip for the layouts ------------------------------------------------------------
static inline uint16_t f16_bits(float x) {
  _Float16 h = (_Float16)x;
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}
struct HiLo { uint16_t hi, lo; };
static inline HiLo split(float v) {           // v = hi + lo to ~22 bits (lo may be an f16 subnormal: the MFMA honours those)
  const float hi = (float)(_Float16)v;
  return {f16_bits(hi), f16_bits(v - hi)};
}

// The item layout [128-channel half][plane hi | lo][tap of kk][channel / 8][128][8] of a conv's weights w (k, cin_pad,
// cout_pad32) times wscale.  map(t, c, &tk, &c2) says where tap t / input channel c of the conv sits among the kernel's
// kk taps and kc_total * 8 channels.
template <typename Map>
static std::vector<uint16_t> pack_items(const jg_op &op, const float *w, float wscale, int kk, int kc_total, int n_half, Map map) {
  const int cin_pad = (op.cin + 1) & ~1, cout_pad32 = (op.cout + 31) / 32 * 32, cout_pad = 128;
  const size_t half_items = (size_t)2 * kk * kc_total * cout_pad;
  std::vector<uint16_t> wh(half_items * n_half * 8, 0);
  for (int t = 0; t < op.k; ++t)
    for (int c = 0; c < op.cin; ++c) {
      int tk, c2;
      map(t, c, &tk, &c2);
      const float *wr = w + ((size_t)t * cin_pad + c) * cout_pad32;
      for (int n0 = 0; n0 < op.cout; n0 += cout_pad) {      // one 128-channel half at a time
        const size_t item = (size_t)(n0 / cout_pad) * half_items + (((size_t)0 * kk + tk) * kc_total + c2 / 8) * cout_pad;
        uint16_t *hi = &wh[item * 8 + c2 % 8], *lo = hi + (size_t)kk * kc_total * cout_pad * 8;   // (the lo plane: kk taps on)
        for (int n = n0; n < std::min(op.cout, n0 + cout_pad); ++n) {
          const HiLo s = split(wr[n] * wscale);
          hi[(n - n0) * 8] = s.hi;
          lo[(n - n0) * 8] = s.lo;
        }
      }
    }
  return wh;
}

// The lane-fragment layout [conv][tap of K][16-channel chunk][plane hi | lo][32-channel output tile][lane][8 halfs] of C-channel
// convs: lane = (cin group of 8) x (output channel of the tile).  val(t, ci, co) is the (scaled) weight.
template <typename Val>
static void pack_lane_frags(std::vector<uint16_t> &frag, int conv, int K, int C, Val val) {
  const int cc_n = C / 16, ct_n = C / 32;
  for (int t = 0; t < K; ++t)
    for (int cc = 0; cc < cc_n; ++cc)
      for (int ct = 0; ct < ct_n; ++ct)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int co = ct * 32 + (lane & 31), ci = cc * 16 + (lane >> 5) * 8 + j;
            const HiLo s = split(val(t, ci, co));
            const size_t base = ((((size_t)conv * K + t) * cc_n + cc) * 2) * ct_n * 64 * 8;
            frag[base + ((size_t)ct * 64 + lane) * 8 + j] = s.hi;
            frag[base + ((size_t)(ct_n + ct) * 64 + lane) * 8 + j] = s.lo;
          }
}

// ---- who reads a slot ------------------------------------------------------------------------------------------------
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

// Walks the ops behind op i while slot `buf` still holds what op i wrote: f(j, reads) sees every op j on the way, the one
// that overwrites the slot last (it may read it first); f returning false ends the walk early.  Returns the index of the
// overwriting op, or the number of ops when the walk ended without one.
template <typename F>
static size_t walk_slot(const jg_model *m, size_t i, int buf, F f) {
  for (size_t j = i + 1; j < m->ops.size(); ++j) {
    if (!f(j, jg_op_reads(m->ops[j], buf))) break;
    if (jg_op_writes(m->ops[j], buf)) return j;
  }
  return m->ops.size();
}

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

// The shape of the family: the conv ops in front of the first pool (convs) and that pool, chained slot to slot and mask to
// mask with the family's geometry, and nothing behind the pool that reads an activation slot.
static bool small_family(const jg_model *m, std::vector<int> &convs, int &pool_op) {
  pool_op = -1;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    if (op.kind == JG_OP_MASK || op.kind == JG_OP_NMD_FINAL) continue;     // (NMD finishes: matched to taps below)
    if (op.kind == JG_OP_CONV) { convs.push_back((int)i); continue; }
    if (op.kind == JG_OP_POOL) { pool_op = (int)i; break; }
    return false;                                   // anything else in front of the pool: not this family
  }
  const int nc = (int)convs.size() - 1;
  if (pool_op < 0 || nc < 1 || !jg_small_supports(nc, m->ops[convs[0]].k, m->vocab)) return false;
  const jg_op &c0 = m->ops[convs[0]];
  if (c0.in_buf != JG_BUF_IDS || c0.cout != 32 || c0.stride != 1 || c0.dilation != 1 || c0.mask_mode != JG_MASK_ANY ||
      !(c0.in_mask == JG_BUF_IDS || c0.in_mask == JG_BUF_NONE))
    return false;
  const bool use_mask = c0.in_mask == JG_BUF_IDS;
  for (int q = 1; q <= nc; ++q) {
    const jg_op &c = m->ops[convs[q]];
    if (c.in_buf != m->ops[convs[q - 1]].out_buf || c.k != 3 || c.cin != 32 || c.cout != 32 || c.stride != 1 ||
        c.dilation != 1 || c.padding != JG_PAD_SAME || c.mask_mode != JG_MASK_ANY || (c.in_mask >= 0) != use_mask)
      return false;
    if (use_mask && c.in_mask != m->ops[convs[q - 1]].out_mask) return false;
  }
  const jg_op &pl = m->ops[pool_op];
  if (pl.in_buf != m->ops[convs[nc]].out_buf || !(pl.arg == JG_POOL_AVG || pl.arg == JG_POOL_MAX) ||
      (pl.in_mask >= 0) != use_mask || (use_mask && pl.in_mask != m->ops[convs[nc]].out_mask))
    return false;
  // no later op may read an activation slot (the kernel never writes them)
  for (size_t i = (size_t)pool_op + 1; i < m->ops.size(); ++i) {
    const int k = m->ops[i].kind;
    if (k == JG_OP_CONV || k == JG_OP_MASK || k == JG_OP_POOL || k == JG_OP_ELTWISE || k == JG_OP_MAXPOOL1D ||
        k == JG_OP_FRAMESUM || k == JG_OP_NMD_FINAL || jg_op_is_mixer(k))
      return false;
  }
  return true;
}

// The epilogue of layer q: folds its BIAS / BN chains and matches  affine [ADD] GELU [affine GELU] [NMD tap]; the first
// affine goes to s1 / t1 (it lives in the weights and the accumulators' initial value: jg_small.hip), the second one and
// the first one's shift to the layer's four rows of epi.  False: the stage list is not the family's.
static bool small_epilogue(const jg_model *m, const float *weights, const std::vector<int> &convs, int q, JgSmallNet *sn,
                           double *s1, double *t1, float *epi) {
  const jg_op &c = m->ops[convs[q]];
  std::vector<double> s2(32, 1.0), t2(32, 0.0);
  auto is_gelu = [&](int st) { return st < c.n_stages && c.stages[st].kind == JG_ST_ACT && c.stages[st].arg == JG_ACT_GELU_TANH; };
  int st = fold_affine(c, 0, weights, 32, s1, t1);
  JgSmallLayer &ly = sn->layer[q];
  if (st < c.n_stages && c.stages[st].kind == JG_ST_ADD) {
    // the shortcut must be the output of an earlier layer of this chain, and the only one alive
    int src = -1;
    for (int r = q - 1; r >= 0; --r)
      if (m->ops[convs[r]].out_buf == c.stages[st].arg) { src = r; break; }
    if (src < 0) return false;
    bool clobbered = false;
    for (int r = src + 1; r < q; ++r) clobbered |= m->ops[convs[r]].out_buf == c.stages[st].arg;
    if (clobbered) return false;
    sn->layer[src].save = 1;
    ly.add = 1;
    ++st;
  }
  if (!is_gelu(st)) return false;
  ++st;
  if (st < c.n_stages && (c.stages[st].kind == JG_ST_BIAS || c.stages[st].kind == JG_ST_BN)) {
    st = fold_affine(c, st, weights, 32, s2.data(), t2.data());
    if (!is_gelu(st)) return false;
    ++st;
    ly.aff2 = 1;
    // (the first layer's accumulators come out of the table phase and its epilogue has no second affine: jg_small.hip)
    if (q == 0) return false;
  }
  if (st < c.n_stages && c.stages[st].kind == JG_ST_NMD && st == c.n_stages - 1) {
    // a tap behind the layer's last stage: masked channel sums of the layer's output, finished by the NMD_FINAL op
    // that reads this partial slot (the program's slot number is kept to find it)
    ly.tap = ++sn->n_taps;
    sn->tap_part_slot[ly.tap] = c.stages[st].arg;
    sn->tap_conv_op[ly.tap] = convs[q];
    ++st;
  }
  if (st != c.n_stages) return false;
  for (int n = 0; n < 32; ++n) {
    epi[0 * 32 + n] = 1.0f;
    epi[1 * 32 + n] = (float)t1[n];
    epi[2 * 32 + n] = (float)s2[n];
    epi[3 * 32 + n] = (float)t2[n];
  }
  return true;
}

// The k = 3 convs' weights times the first affine's scale as split-f16 lane fragments.  They go into f16 planes WITHOUT a
// power-of-two pre-scale: they must sit inside the f16 range (a large batch-norm scale would turn hi into inf and lo into
// -inf: NaN logits), and the layer's largest weight must stay well above the subnormal quantum 2^-24 the lo plane resolves
// (hi + lo then still carries ~19 bits of it); otherwise (false) the model stays on the generic split-f16 / exact-f32
// kernels, which pre-scale per conv.
static bool small_fragments(const jg_model *m, const float *weights, const std::vector<int> &convs, const std::vector<double> &scale1,
                            std::vector<uint16_t> &frag) {
  for (int q = 1; q < (int)convs.size(); ++q) {
    const float *w = weights + m->ops[convs[q]].w_off;   // (3, 32, 32) f32 (cin even, cout multiple of 32: no padding)
    auto scaled = [&](int t, int ci, int co) { return (double)w[((size_t)t * 32 + ci) * 32 + co] * scale1[(size_t)q * 32 + co]; };
    double vmax = 0.0;
    bool ok = true;
    for (int t = 0; t < 3; ++t)
      for (int ci = 0; ci < 32; ++ci)
        for (int co = 0; co < 32; ++co) {
          const double v = std::fabs(scaled(t, ci, co));
          if (!(v <= 65000.0)) ok = false;            // (also catches NaN)
          vmax = std::max(vmax, v);
        }
    if (vmax != 0.0 && vmax < 0.015625) ok = false;
    if (!ok) return false;
    pack_lane_frags(frag, q - 1, 3, 32, [&](int t, int ci, int co) { return (float)scaled(t, ci, co); });
  }
  return true;
}

int jg_prepare_small(jg_model *m, const float *weights) {
  std::vector<int> convs;
  int pool_op;
  if (!small_family(m, convs, pool_op)) return JG_OK;
  const int nc = (int)convs.size() - 1;
  const jg_op &c0 = m->ops[convs[0]], &pl = m->ops[pool_op];
  const bool use_mask = c0.in_mask == JG_BUF_IDS;
  JgSmallNet *sn = new JgSmallNet();
  for (JgSmallLayer &ly : sn->layer) ly.add = ly.aff2 = ly.save = ly.tap = 0;
  std::vector<float> epi((size_t)(nc + 1) * 4 * 32, 0.f);
  std::vector<uint16_t> frag((size_t)nc * 12 * 64 * 8, 0);
  std::vector<double> scale1((size_t)(nc + 1) * 32, 1.0), shift1((size_t)(nc + 1) * 32, 0.0);
  bool ok = true;
  for (int q = 0; q <= nc && ok; ++q)
    ok = small_epilogue(m, weights, convs, q, sn, &scale1[(size_t)q * 32], &shift1[(size_t)q * 32], &epi[(size_t)q * 4 * 32]);
  ok = ok && small_fragments(m, weights, convs, scale1, frag);
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
  // first-layer table T_t[id] = E[id] . W_t (f64) times the first affine's scale, row `vocab` = zeros (padding), row 0 =
  // zeros when ids mask
  const int k0 = c0.k, vr = m->vocab + 1, cin_pad = (c0.cin + 1) & ~1;
  std::vector<float> lut((size_t)k0 * vr * 32, 0.f);
  for (int t = 0; t < k0; ++t)
    for (int id = (use_mask ? 1 : 0); id < m->vocab; ++id)
      for (int n = 0; n < 32; ++n)
        lut[((size_t)t * vr + id) * 32 + n] =
            (float)(first_layer_dot(weights + c0.b_off, weights + c0.w_off, id, t, n, c0.cin, cin_pad, 32) * scale1[(size_t)n]);
  // every output position reads exactly one row of tap 0 (a codon's, the masked id 0's or the padding row `vocab`):
  // the first affine's shift rides on all of them
  for (int id = 0; id < vr; ++id)
    for (int n = 0; n < 32; ++n) lut[(size_t)id * 32 + n] = (float)((double)lut[(size_t)id * 32 + n] + shift1[(size_t)n]);
  JG_HIP(upload(m, KEY_SMALL, lut, &sn->d_lut));
  JG_HIP(upload(m, KEY_SMALL, epi, &sn->d_epi));
  JG_HIP(upload(m, KEY_SMALL, frag, &sn->d_wfrag));

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
      for (int n = 0; n < c.cout; ++n)
        tab[((size_t)t * V + id) * cq * 4 + n] = (float)first_layer_dot(emb, w, id, t, n, c.cin, cin_pad, cout_pad);
  if (bias_off >= 0)
    for (int n = 0; n < c.cout; ++n) bias[(size_t)n] = weights[bias_off + n];
  JG_HIP(upload(m, KEY_TABNET, tab, &m->tab_table));
  JG_HIP(upload(m, KEY_TABNET, bias, &m->tab_bias));
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
            const HiLo s = split(tab[((size_t)tap * V + (nuc + 1)) * cq * 4 + co]);
            const size_t base = (((size_t)tile * ks + st) * 2) * 64 * 8;
            frag[base + (size_t)lane * 8 + j] = s.hi;
            frag[base + 64 * 8 + (size_t)lane * 8 + j] = s.lo;
          }
    std::vector<float> b512(512, 0.f);
    for (int n = 0; n < c.cout; ++n) b512[(size_t)n] = bias[(size_t)n];
    JG_HIP(upload(m, KEY_TABNET, frag, &m->tab_wfrag));
    JG_HIP(upload(m, KEY_TABNET, b512, &m->tab_bias512));
  }
  m->tab_conv = 0;
  m->tab_pool = 1;
  m->tab_act = act;
  m->tab_cq = cq;
  m->tab_vocab = V;
  m->tab_zero = row0_zero ? 0 : m->vocab;
  return JG_OK;
}

// exact-f32 conv operands: weights grouped by 8 input channels so that a lane fetches the four
// k-steps of a group with one 16-byte load (see conv_f32_kernel)
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
    JG_HIP(upload(m, i, w8, &m->hprep[i].d_w8));
  }
  return JG_OK;
}

// ---------------------------------------------------------------------------
// jg_prepare_f16, stage by stage: one conv on the split-f16 kernel
// ---------------------------------------------------------------------------
struct ConvGeom {                 // what conv_geometry derives for the stages behind it
  int kk, kdil;                   // taps and dilation of the kernel that carries the conv
  int cin16, cwide;               // input channels padded to 16, output channels incl. zero padding (n_half x 128)
  bool lut_ok, mfma_ok;           // the first-layer table variant / the MFMA tiling can run it
};

// Stage 1 - eligibility by geometry alone: which kernel carries the conv (a 1x1 .. 4-tap conv rides the 5-tap kernel,
// stride 2 runs as the stride-1 conv whose even outputs are kept, a first conv on ids as the table variant when the table
// fits LDS), and are its taps, dilation and widths inside that kernel's tiling?  Returns the refusal text, or null with
// the derived sizes in g and hp (as_k5, cc_in, n_half, cw).
static const char *conv_geometry(const jg_model *m, size_t i, ConvHPrep &hp, ConvGeom &g) {
  const jg_op &op = m->ops[i];
  if ((int)i == m->tab_conv) return "runs as the table-net kernel (exact f32, ids to pooled vectors)";
  // a 1x1 conv (the bypass of a strided / widening residual block) and a 3-tap conv (ResidualBlock's default kernel
  // size, layers.py:1787) ride the 5-tap kernel: weights in the middle taps, the matrix-core work of the others skipped
  hp.as_k5 = op.k >= 1 && op.k <= 4 && op.in_buf != JG_BUF_IDS;       // (2- and 4-tap convs the same way)
  g.kk = hp.as_k5 ? 5 : op.k;
  g.kdil = (hp.as_k5 && op.k == 1) ? 1 : op.dilation;
  if (op.stride != 1 && !(op.stride == 2 && (g.kk == 5 || g.kk == 7 || g.kk == 9) && op.in_buf != JG_BUF_IDS)) return "strided conv";
  // (a first conv on ids runs as the table variant whatever its tap count, when the table fits LDS)
  static const bool no_lut = jg_exp_env("JG_NO_LUT") != nullptr;
  g.lut_ok = !no_lut && op.in_buf == JG_BUF_IDS && (op.in_mask == JG_BUF_IDS || op.in_mask < 0) && op.cout <= 128 &&
             op.stride == 1 && jg_conv_lut_supports(op.k, op.dilation, m->vocab);
  g.mfma_ok = jg_conv_f16_supports(g.kk, g.kdil);
  if (!g.mfma_ok && !g.lut_ok) return "taps / dilation outside the split-f16 tiling";
  const bool narrow = op.cout == 32 || op.cout == 64;
  if (op.cout % 16 != 0 || !(narrow || (op.cout > 64 && op.cout <= 128) || op.cout % 128 == 0))
    return "conv width is not 32, 64, 80..128 or a multiple of 128 channels";
  // (the k = 5, 7 and 9 kernels are all built with run-time output geometry - other widths than 128, stride 2; a first
  // conv of up to 128 channels runs as the table variant, which has it too: no table -> 128 channels only, stage 5)
  if (op.in_buf == JG_BUF_IDS && op.cout > 128) return "first conv wider than 128 channels";
  if (op.in_buf != JG_BUF_IDS && op.cin % 16 != 0) return "conv input width is not a multiple of 16";
  g.cin16 = (op.cin + 15) / 16 * 16;
  hp.cc_in = g.cin16 / 16;
  hp.n_half = (op.cout + 127) / 128;
  hp.cw = (narrow && op.in_buf != JG_BUF_IDS) ? op.cout : 128;    // (a first conv runs as the table variant: 128-wide)
  g.cwide = hp.n_half * 128;
  return nullptr;
}

// Stage 2 - the operands of the matrix-core loop: the power-of-two scale that brings the largest weight into [4, 8)
// (hp.acc_scale undoes it in the epilogue), the weights times it as hi / lo item planes, and for a conv on ids the
// embedding as hi / lo planes [vocab][cin16/16][plane][8-channel half][8] - refused (*why) when a value leaves the f16 range.
static int conv_operands(jg_model *m, size_t i, const float *weights, const ConvGeom &g, const char **why) {
  const jg_op &op = m->ops[i];
  ConvHPrep &hp = m->hprep[i];
  const float *w = weights + op.w_off;   // (k, cin_pad, cout_pad32) f32
  const int cin_pad = (op.cin + 1) & ~1, cout_pad32 = (op.cout + 31) / 32 * 32;
  float maxabs = 0.f;
  for (int64_t q = 0; q < (int64_t)op.k * cin_pad * cout_pad32; ++q) maxabs = std::max(maxabs, fabsf(w[q]));
  int sexp = 0;
  if (maxabs > 0.f) {
    int e2;
    frexpf(maxabs, &e2);            // maxabs = f * 2^e2, f in [0.5, 1)
    sexp = 3 - e2;                  // scaled max in [4, 8)
  }
  hp.acc_scale = ldexpf(1.f, -sexp);
  const int kc_total = g.cin16 / 8;
  hp.wh_half_items = (int64_t)2 * g.kk * kc_total * 128;       // one 128-channel half: [plane][tap][kc][128]
  const int tap0 = hp.as_k5 ? std::max(1, (5 - op.k) / 2) : 0;   // (a 1x1 / 3-tap conv's taps sit in the middle of five)
  const std::vector<uint16_t> wh = pack_items(op, w, ldexpf(1.f, sexp), g.kk, kc_total, hp.n_half,
                                              [&](int t, int c, int *tk, int *c2) { *tk = tap0 + t; *c2 = c; });
  JG_HIP(upload(m, i, wh, &hp.d_wh));
  if (op.in_buf != JG_BUF_IDS) return JG_OK;
  const float *emb = weights + op.b_off;   // (vocab, cin)
  std::vector<uint16_t> eh((size_t)m->vocab * hp.cc_in * 4 * 8, 0);
  for (int id = 0; id < m->vocab; ++id)
    for (int c = 0; c < op.cin; ++c) {
      const float v = emb[(size_t)id * op.cin + c];
      const HiLo s = split(v);
      if (!(fabsf(v) <= 65000.f)) *why = "embedding value outside the f16 range";
      const int cc = c / 16, hh = (c % 16) / 8, j = c % 8;
      eh[(((size_t)id * hp.cc_in + cc) * 4 + 0 * 2 + hh) * 8 + j] = s.hi;
      eh[(((size_t)id * hp.cc_in + cc) * 4 + 1 * 2 + hh) * 8 + j] = s.lo;
    }
  JG_HIP(upload(m, i, eh, &hp.d_embh));
  return JG_OK;
}

// Stage 3 - the epilogue as the kernel sees it: bias / batch-norm chains (and, first, the weights' un-scale) folded into
// per-channel affines, every other stage as one entry of the host stage list hp.hst, and the parameter rows they index -
// returned as [hp.n_epi_rows][scale | shift][cwide].  Refuses (*why, the first reason) stage kinds and counts the kernel has
// no room for; a conv refused before it gets no stage list.
static std::vector<float> conv_epilogue(const jg_op &op, const float *weights, int cwide, ConvHPrep &hp, const char **why) {
  std::vector<float> tab;
  auto fail = [&](const char *w) { if (*why == nullptr) *why = w; };
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
  for (int q = 0; q < op.n_stages && *why == nullptr;) {
    const int behind = fold_affine(op, q, weights, op.cout, sc.data(), sh.data());
    if (behind > q) { pending = true; q = behind; continue; }
    const jg_stage &st = op.stages[q++];
    flush();
    if (hp.n_hst >= JG_MAX_STAGES) { fail("epilogue too long"); break; }
    HStageArg h{0, st.arg, st.f0, 0};
    switch (st.kind) {
      case JG_ST_DYT:
        h.kind = JG_HST_DYT;
        h.pad_ = hp.n_epi_rows++;
        for (int n = 0; n < cwide; ++n) tab.push_back(n < op.cout ? (weights + st.p2)[n] : 0.f);
        for (int n = 0; n < cwide; ++n) tab.push_back(n < op.cout ? (weights + st.p3)[n] : 0.f);
        break;
      case JG_ST_ADD: h.kind = JG_HST_ADD; hp.add_slot = st.arg; break;
      case JG_ST_ACT: h.kind = JG_HST_ACT; break;
      case JG_ST_NMD:
        h.kind = JG_HST_NMD;
        if (hp.nmd_slot < 0) hp.nmd_slot = st.arg;
        else if (hp.nmd_slot2 < 0) hp.nmd_slot2 = st.arg;
        else fail("more than two NMD taps in one conv");
        break;
      case JG_ST_MASKMUL: h.kind = JG_HST_MASKMUL; break;
      default: fail("epilogue stage not supported by the split-f16 kernel"); break;
    }
    hp.hst[hp.n_hst++] = h;
  }
  if (*why == nullptr) {
    if (pending && hp.n_hst >= JG_MAX_STAGES) fail("epilogue too long");
    else flush();
  }
  if (hp.n_epi_rows > JG_EPI_ROWS) fail("more norm stages than the split-f16 epilogue table holds");
  return tab;
}

// Stage 4 - which compiled epilogue runs the stage list.  The canonical order is
//   affine [nmd] [norm1] [add] [gelu] [nmd] [norm2] [gelu]
// with one activation kind per conv (the DyT patterns are compiled for the tanh-GELU only): a list in that order is its
// JG_EP_* bits (ep), any other JG_EP_GENERIC.  A canonical list without an instantiation of its own for this conv's
// geometry (or with two NMD taps, which need the second accumulator) runs on the run-time-flag epilogue (ep =
// JG_EP_RUNTIME, the bits in ep_rt) - tanh-GELU lists only: it carries every stage kind at once, the erf / ReLU forms
// beside them spill.  Host decisions alone: nothing here needs the weights or the device.
struct EpMatch {
  unsigned ep = JG_EP_GENERIC, ep_rt = 0;
  int act_kind = JG_ACT_GELU_TANH;
  float alpha1 = 0.f, alpha2 = 0.f;
  int dytmask1 = 0, dytmask2 = 0;
};
static EpMatch match_epilogue(const HStageArg *hst, int n, const jg_op &op, bool as_k5, bool two_taps) {
  EpMatch r;
  unsigned ep = 0;
  int q = 0;
  auto is = [&](int kind) { return q < n && hst[q].kind == kind; };
  bool ok = is(JG_HST_AFFINE);
  if (ok) {
    ++q;
    if (is(JG_HST_NMD)) { ep |= JG_EP_NMD1; ++q; }
    if (is(JG_HST_AFFINE)) { ep |= JG_EP_NORM1_AFF; ++q; }
    else if (is(JG_HST_DYT)) { ep |= JG_EP_NORM1_DYT; r.alpha1 = hst[q].f0; r.dytmask1 = hst[q].arg; ++q; }
    if (is(JG_HST_ADD)) { ep |= JG_EP_ADD; ++q; }
    int gelu_kind = 0;   // all activation stages of a compiled pattern share one kind
    auto is_gelu = [&]() {
      if (!is(JG_HST_ACT)) return false;
      const int k = hst[q].arg;
      if (k != JG_ACT_GELU_TANH && k != JG_ACT_GELU_ERF && k != JG_ACT_RELU) return false;
      if (gelu_kind != 0 && gelu_kind != k) return false;
      gelu_kind = k;
      return true;
    };
    if (is_gelu()) { ep |= JG_EP_ACT1; ++q; }
    if (is(JG_HST_NMD)) { ep |= JG_EP_NMD2; ++q; }
    if (is(JG_HST_AFFINE)) { ep |= JG_EP_NORM2_AFF; ++q; }
    else if (is(JG_HST_DYT)) { ep |= JG_EP_NORM2_DYT; r.alpha2 = hst[q].f0; r.dytmask2 = hst[q].arg; ++q; }
    if (is_gelu()) { ep |= JG_EP_ACT2; ++q; }
    ok = q == n;
    r.act_kind = gelu_kind != 0 ? gelu_kind : JG_ACT_GELU_TANH;
  }
  if (ok && (ep & (JG_EP_NORM1_DYT | JG_EP_NORM2_DYT)) && (ep & (JG_EP_ACT1 | JG_EP_ACT2)) && r.act_kind != JG_ACT_GELU_TANH)
    ok = false;
  r.ep = ok ? ep : JG_EP_GENERIC;
  const bool on_ids = op.in_buf == JG_BUF_IDS;
  const bool narrow_geo = !on_ids && (op.cout != 128 || op.stride != 1 || as_k5);
  if (ok && r.act_kind == JG_ACT_GELU_TANH && !(ep & JG_EP_ADD && on_ids) &&
      (!jg_conv_f16_has_pattern(ep, on_ids) || (narrow_geo && !jg_conv_f16_has_narrow_pattern(ep)) ||
       ((ep & JG_EP_NMD1) && (ep & JG_EP_NMD2)))) {
    r.ep_rt = ep;
    r.ep = JG_EP_RUNTIME;
  }
  if (r.ep != JG_EP_RUNTIME && two_taps) r.ep = JG_EP_GENERIC;   // two taps need the second accumulator
  return r;
}

// Stage 5 - a first conv on ids as a sum of k table rows T_t[id] = E[id] . W_t (f64 on the host): the kernel's table
// variant needs no matrix cores and no acc un-scale, so its epilogue table is the conv's (tab) with row 0's scale
// divided by acc_scale again.  Table [64-channel half][tap][vocab + the all-zero padding row][64].
static int conv_first_layer_table(jg_model *m, size_t i, const float *weights, const std::vector<float> &tab) {
  const jg_op &op = m->ops[i];
  ConvHPrep &hp = m->hprep[i];
  const int vr = m->vocab + 1, cin_pad = (op.cin + 1) & ~1, cout_pad32 = (op.cout + 31) / 32 * 32;
  std::vector<float> lut((size_t)2 * op.k * vr * 64, 0.f);
  for (int t = 0; t < op.k; ++t)
    for (int id = (op.in_mask == JG_BUF_IDS ? 1 : 0); id < m->vocab; ++id)   // id 0 is masked: zero row
      for (int n = 0; n < op.cout; ++n)
        lut[(((size_t)(n >> 6) * op.k + t) * vr + id) * 64 + (n & 63)] =
            (float)first_layer_dot(weights + op.b_off, weights + op.w_off, id, t, n, op.cin, cin_pad, cout_pad32);
  std::vector<float> tab_lut(tab);
  for (int n = 0; n < 128; ++n) tab_lut[n] = (float)((double)tab[n] / (double)hp.acc_scale);   // row 0 scale
  JG_HIP(upload(m, i, lut, &hp.d_lut));
  JG_HIP(upload(m, i, tab_lut, &hp.d_epi_lut));
  return JG_OK;
}

// One conv through the stages; hp.f16_ok says whether it came through all of them.  Only compiled stage patterns run on
// the split-f16 path: the interpreted epilogue was measured 12x slower than the compiled ones (and 3x slower than the
// exact-f32 kernels), so anything else stays on the exact-f32 path.
static int prepare_conv_f16(jg_model *m, size_t i, const float *weights, std::string *first_reason) {
  const jg_op &op = m->ops[i];
  ConvHPrep &hp = m->hprep[i];
  ConvGeom g;
  hp.f16_ok = false;
  const char *why = conv_geometry(m, i, hp, g);      // the first reason this conv stays on the exact-f32 kernel
  bool conv_ok = why == nullptr;
  auto cfail = [&](const char *w) {
    conv_ok = false;
    if (why == nullptr) why = w;
  };
  if (conv_ok) {
    int rc = conv_operands(m, i, weights, g, &why);
    if (rc != JG_OK) return rc;
    const std::vector<float> tab = conv_epilogue(op, weights, g.cwide, hp, &why);
    conv_ok = why == nullptr;
    const EpMatch em = match_epilogue(hp.hst, hp.n_hst, op, hp.as_k5, hp.nmd_slot2 >= 0);
    hp.ep = em.ep; hp.ep_rt = em.ep_rt; hp.act_kind = em.act_kind;
    hp.alpha1 = em.alpha1; hp.alpha2 = em.alpha2; hp.dytmask1 = em.dytmask1; hp.dytmask2 = em.dytmask2;
    if (conv_ok && !jg_conv_f16_has_pattern(hp.ep, op.in_buf == JG_BUF_IDS)) {
      cfail("a conv's stage list is not one of the compiled split-f16 epilogue patterns");
    }
    if (conv_ok && op.in_buf != JG_BUF_IDS && (op.cout != 128 || op.stride != 1 || hp.as_k5) && !jg_conv_f16_has_narrow_pattern(hp.ep))
      cfail("the stage list of a conv of other than 128 channels / stride 1 is not one of the patterns compiled for it");
    if (conv_ok && op.stride == 2 && ((hp.ep == JG_EP_RUNTIME ? hp.ep_rt : hp.ep) & (JG_EP_ADD | JG_EP_NMD1 | JG_EP_NMD2)))
      cfail("strided conv with a shortcut or an NMD tap in its epilogue");
    if (conv_ok) {
      std::vector<float> th(tab.size());                 // [half][row][2][128]
      const int nr = hp.n_epi_rows;
      for (int hf = 0; hf < hp.n_half; ++hf)
        for (int r = 0; r < nr * 2; ++r)
          for (int n = 0; n < 128; ++n) th[((size_t)hf * nr * 2 + r) * 128 + n] = tab[(size_t)r * g.cwide + hf * 128 + n];
      JG_HIP(upload(m, i, th, &hp.d_epi));
    }
    if (conv_ok && g.lut_ok && (rc = conv_first_layer_table(m, i, weights, tab)) != JG_OK) return rc;
    if (conv_ok && op.in_buf == JG_BUF_IDS && hp.d_lut == nullptr && (op.cout != 128 || !g.mfma_ok))
      cfail("first conv without the table variant is not a 128-channel 5- / 7- / 9-tap conv");
  }
  if (why != nullptr) {
    if (first_reason->empty()) *first_reason = why;
    hp.why_f32 = why;
  }
  hp.f16_ok = conv_ok;
  return JG_OK;
}

// The output of split-f16 conv i: F16S when its first reader wants that, f32 rows otherwise - and no tensor at all when
// the only reader of the f32 output is a masked global max pool over the conv's own output mask: the conv reduces in its
// epilogue instead of storing 4 B per element and reading it back (hp.pool_op, m->pool_fused_by).
static void plan_conv_output(jg_model *m, size_t i) {
  const jg_op &op = m->ops[i];
  ConvHPrep &hp = m->hprep[i];
  int readers = 0, pool_idx = -1;
  walk_slot(m, i, op.out_buf, [&](size_t j, bool reads) {
    const jg_op &o = m->ops[j];
    if (!reads || o.kind == JG_OP_NMD_FINAL) return true;       // (NMD_FINAL only takes the slot's shape: no format is asked of it)
    if (readers++ == 0)                                          // the first reader: does it read the slot as an F16S tensor?
      hp.out_f16s = (o.kind == JG_OP_MAXPOOL1D && o.in_buf == op.out_buf) || (o.kind == JG_OP_CONV && m->hprep[j].f16_ok);
    pool_idx = (o.kind == JG_OP_POOL && o.arg == JG_POOL_MAX && o.in_mask == op.out_mask) ? (int)j : -2;
    return true;
  });
  if (hp.out_f16s || jg_exp_env("JG_NO_POOL_FUSE") != nullptr) return;
  if (readers == 1 && pool_idx >= 0) {
    hp.pool_op = pool_idx;
    m->pool_fused_by[(size_t)pool_idx] = (int)i;
  }
}

// Tensor formats.  Walks the program with the format of every activation slot (f32 rows or F16S items): split-f16 convs
// read and write F16S (f32 when the next reader needs it, or no tensor at all when only a max pool reads it), everything
// else works on f32; where a reader meets the other format, a layout conversion is queued in front of it (run_chunk
// converts into a scratch tensor and swaps the slot's pointer).  Ineligible convs (1x1 bypass, other strides or widths)
// keep the exact-f32 kernel inside an otherwise split-f16 program; without any eligible conv the model has no fast path.
static int jg_plan_formats(jg_model *m, const std::string &first_reason) {
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
  auto need_inputs = [&](size_t i, bool want_f32) {      // the op's input and the shortcuts its stages add
    const jg_op &op = m->ops[i];
    need(i, op.in_buf, want_f32);
    for (int q = 0; q < op.n_stages; ++q)
      if (op.stages[q].kind == JG_ST_ADD) need(i, op.stages[q].arg, want_f32);
  };
  for (size_t i = 0; i < m->ops.size(); ++i) {
    const jg_op &op = m->ops[i];
    ConvHPrep &hp = m->hprep[i];
    switch (op.kind) {
      case JG_OP_CONV:
        need_inputs(i, !hp.f16_ok);
        if (hp.f16_ok) plan_conv_output(m, i);
        is_f32[op.out_buf] = !hp.out_f16s;
        break;
      case JG_OP_EMBED:
        is_f32[op.out_buf] = true;                      // the lookup writes f32 rows: the first conv converts if it wants F16S
        break;
      case JG_OP_ELTWISE:
        need_inputs(i, true);
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

// Every conv on its own: can it run on the split-f16 kernel (taps / dilation inside the tiling, a compiled epilogue
// pattern; 32, 64 or a multiple of 128 output channels - narrow convs on 64- / 32-channel workgroup tiles, wider ones as
// one launch per 128 channels; stride 2 as the stride-1 conv whose even outputs are kept)?  Then the formats between them.
int jg_prepare_f16(jg_model *m, const float *weights) {
  m->hprep.assign(m->ops.size(), ConvHPrep());
  m->pool_fused_by.assign(m->ops.size(), -1);
  m->f16_eligible = true;
  m->f16_reason.clear();
  std::string first_reason;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    if (m->ops[i].kind != JG_OP_CONV) continue;
    const int rc = prepare_conv_f16(m, i, weights, &first_reason);
    if (rc != JG_OK) return rc;
  }
  return jg_plan_formats(m, first_reason);
}

// Stride-2 convs without dropped work.  A strided residual block (layers.py:1882-1915: conv1 of 5 taps and the
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
  for (size_t p = 0; p < m->ops.size(); ++p) {
    const jg_op &po = m->ops[p];
    ConvHPrep &pp = m->hprep[p];
    if (po.kind != JG_OP_CONV || !pp.f16_ok || !pp.out_f16s || pp.pool_op >= 0 || po.stride != 1 || po.out_buf < 0 ||
        po.cout % 16 != 0 || (int)p == m->tab_conv || po.in_buf == JG_BUF_IDS ||
        !jg_conv_f16_has_narrow_pattern(pp.ep))           // (the store is built into the run-time-geometry tiles)
      continue;
    std::vector<size_t> readers;
    bool ok = true, mask_rewritten = false;
    walk_slot(m, p, po.out_buf, [&](size_t j, bool reads) {
      const jg_op &o = m->ops[j];
      if (reads) {
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
      return ok;
    });
    if (!ok || readers.empty()) continue;
    // weights of the 5-tap readers, re-arranged for both parities of the input length
    bool built = true;
    for (size_t j : readers) {
      const jg_op &o = m->ops[j];
      ConvHPrep &hr = m->hprep[j];
      if (o.k != 5) continue;
      const float wscale = 1.0f / hr.acc_scale;            // the conv's own power-of-two scale (the epilogue table undoes it)
      const int kk = 5, kc_total = 2 * o.cin / 8;
      hr.ps_half_items = (int64_t)2 * kk * kc_total * 128;
      for (int par = 0; par < 2 && built; ++par) {          // par = input length & 1
        const int pl = par ? 2 : 1;
        const std::vector<uint16_t> wh = pack_items(o, weights + o.w_off, wscale, kk, kc_total, hr.n_half, [&](int t, int c, int *tk, int *c2) {
          const int q = t - pl, ph = ((q % 2) + 2) % 2, off3 = (q - ph) / 2 + 1;     // phase, tap of the 3-tap conv (0 .. 2)
          *tk = 1 + off3;                                                            // ... in the middle of the kernel's five
          *c2 = ph * o.cin + c;
        });
        built = upload(m, j, wh, &hr.d_wh_ps[par]) == hipSuccess;
      }
      if (!built) break;
    }
    if (!built) {
      (void)hipGetLastError();
      for (size_t j : readers)
        for (int par = 0; par < 2; ++par) release(m, &m->hprep[j].d_wh_ps[par]);
      continue;
    }
    pp.ps_store = true;
    for (size_t j : readers) m->hprep[j].ps_read = m->ops[j].k == 5 ? 1 : 2;
  }
  return JG_OK;
}

// Whole narrow residual blocks as one launch (jg_resblock.hip).  conv1 [bias, norm, GELU] and conv2 [bias, norm,
// + block input, GELU] of a stride-1 block without bypass (layers.py:1882-1915), 32 or 64 channels, five taps, one dilation:
// the intermediate tensor lives in LDS only.  conv1's op is skipped at run time, conv2's launch computes both; the mask ops
// between them run as before (the kernel reads conv2's input mask from their output).
// Is conv ia the conv1 of such a block?  Returns its conv2, or the number of ops.
static size_t resblock_second(const jg_model *m, size_t ia) {
  const size_t n = m->ops.size();
  const jg_op &A = m->ops[ia];
  const ConvHPrep &ha = m->hprep[ia];
  if (A.kind != JG_OP_CONV || !ha.f16_ok || ha.rb_second >= 0 || ha.rb_first >= 0 || A.in_buf < 0 || A.stride != 1 ||
      A.padding != JG_PAD_SAME || A.cin != A.cout || !(jg_resblock_supports(A.cout, A.k, A.dilation) || jg_resblock64_supports(A.cout, A.k, A.dilation)) || !ha.out_f16s ||
      ha.ep != JG_EP_ACT1 || ha.act_kind != JG_ACT_GELU_TANH || ha.pool_op >= 0 || ha.ps_store || ha.ps_read != 0 ||
      ha.n_cvt != 0 || (int)ia == m->tab_conv)
    return n;
  // the only reader of conv1's output: conv2, before anything overwrites it (mask ops may sit in between)
  size_t ib = n;
  bool ok = true;
  const size_t writer = walk_slot(m, ia, A.out_buf, [&](size_t j, bool reads) {
    if (!reads) return true;
    if (ib == n && m->ops[j].kind == JG_OP_CONV && m->ops[j].in_buf == A.out_buf) ib = j;
    else ok = false;
    return true;
  });
  if (!ok || ib == n || writer == ib) return n;                              // (conv2 in place: not a residual block)
  for (size_t j = ia + 1; j < ib && ok; ++j)                               // nothing but mask ops between the two
    ok = m->ops[j].kind == JG_OP_MASK && m->ops[j].out_mask != A.in_mask && m->ops[j].out_mask != A.out_mask;
  const jg_op &B = m->ops[ib];
  const ConvHPrep &hb = m->hprep[ib];
  if (!ok || !hb.f16_ok || B.stride != 1 || B.padding != JG_PAD_SAME || B.k != A.k || B.dilation != A.dilation ||
      B.cin != A.cout || B.cout != A.cout || B.in_mask != A.out_mask || !hb.out_f16s ||
      hb.ep != (JG_EP_ADD | JG_EP_ACT1) || hb.act_kind != JG_ACT_GELU_TANH || hb.add_slot != A.in_buf ||
      B.out_buf == A.in_buf || B.out_buf == A.out_buf || hb.pool_op >= 0 || hb.ps_read != 0 || hb.n_cvt != 0 ||
      hb.nmd_slot >= 0 || ha.nmd_slot >= 0)
    return n;
  return ib;
}

int jg_plan_resblocks(jg_model *m, const float *weights) {
  if (!m->f16_eligible) return JG_OK;
  static const bool off = jg_exp_env("JG_NO_RESBLOCK") != nullptr;
  if (off) return JG_OK;
  for (size_t ia = 0; ia < m->ops.size(); ++ia) {
    const size_t ib = resblock_second(m, ia);
    if (ib == m->ops.size()) continue;
    ConvHPrep &ha = m->hprep[ia], &hb = m->hprep[ib];
    // both convs' weights as lane fragments, and per conv the affine in front of its first other stage (bias / batch norm
    // folded with the weights' un-scale): [conv][scale | shift][C]
    const int C = m->ops[ia].cout, K = m->ops[ia].k;
    std::vector<uint16_t> frag((size_t)2 * K * (C / 16) * 2 * (C / 32) * 64 * 8, 0);
    std::vector<float> epi((size_t)4 * C, 0.f);
    bool range_ok = true;
    for (int c = 0; c < 2; ++c) {
      const jg_op &op = m->ops[c == 0 ? ia : ib];
      const ConvHPrep &hp = c == 0 ? ha : hb;
      const float *w = weights + op.w_off;                 // (k, cin_pad, cout_pad32)
      const int cin_pad = (op.cin + 1) & ~1, cout_pad32 = (op.cout + 31) / 32 * 32;
      const float wscale = 1.0f / hp.acc_scale;
      pack_lane_frags(frag, c, K, C, [&](int t, int ci, int co) {
        const float v = w[((size_t)t * cin_pad + ci) * cout_pad32 + co] * wscale;
        if (!(fabsf(v) <= 65000.f)) range_ok = false;
        return v;
      });
      std::vector<double> s((size_t)C, (double)hp.acc_scale), t((size_t)C, 0.0);
      fold_affine(op, 0, weights, C, s.data(), t.data());
      for (int n = 0; n < C; ++n) { epi[(size_t)(c * 2) * C + n] = (float)s[(size_t)n]; epi[(size_t)(c * 2 + 1) * C + n] = (float)t[(size_t)n]; }
    }
    if (!range_ok) continue;
    if (upload(m, ib, frag, &hb.d_rb_wfrag) != hipSuccess || upload(m, ib, epi, &hb.d_rb_epi) != hipSuccess) {
      (void)hipGetLastError();
      release(m, &hb.d_rb_wfrag);
      release(m, &hb.d_rb_epi);
      continue;
    }
    ha.rb_second = (int)ib;
    hb.rb_first = (int)ia;
  }
  return JG_OK;
}
