// C-ABI of libjaeger_hip.so, ingest part: the window encoder (jg_encode) and jg_predict_windows - bases to outputs,
// whole-buffer or streamed through two staging spans.  The forward passes themselves are jg_run.hip's.
#include <thread>

#include "jg_host.h"

static int frame_len(int nt) {
  if (nt < 3) return 0;
  const int off = (nt % 3 == 0) ? -2 : ((nt % 3 == 1) ? -1 : 0);
  const int usable = nt - 5 + off;
  return usable > 0 ? (usable + 2) / 3 : 0;
}

// shared by jg_encode / jg_predict_windows: stage host-side window tables and
// run the encoder into a device id tensor
static int encode_common(jg_engine *e, jg_model *scratch_owner, const uint8_t *bases, int64_t n_bases,
                         int bases_loc, const int64_t *win_start, const int32_t *win_len, int win_loc,
                         int64_t n_win, int32_t fsize, const uint8_t *lut65, int32_t flags,
                         int32_t l_pad, uint8_t *d_ids, int32_t *d_counts, uint8_t *d_lut,
                         std::vector<void *> &to_free, hipStream_t s) {
  // scratch_owner: a model whose grow-only device buffers hold the uploaded bases / window table (no hipMalloc / hipFree
  // per call); without one (jg_encode) the copies are temporary
  // l_pad must hold the longest frame: known exactly for host-side window tables (the short-contig
  // pass pads to the longest window of a batch, commands/predict.py:236-245), fsize-derived otherwise
  const bool nt_ids = (flags & JG_ENC_NUCLEOTIDE) != 0;       // a row holds bases, not codons
  const bool di_ids = (flags & JG_ENC_DICODON) != 0;          // ... or codon pairs (six bases apart)
  JG_REQUIRE(!(nt_ids && di_ids), JG_ERR_INVALID, "encode: nucleotide and dicodon ids are different encodings");
  auto row_len = [&](int n) {                                  // entries per frame of a window cropped to n bases
    const int off3 = (fsize % 3 == 0) ? -2 : ((fsize % 3 == 1) ? -1 : 0);
    if (di_ids) { const int u = n - 8 + off3; return u > 0 ? (u + 5) / 6 : 0; }
    const int u = n - 5 + off3;
    return u > 0 ? (u + 2) / 3 : 0;
  };
  int need = nt_ids ? fsize : (di_ids ? row_len(fsize) : frame_len(fsize));
  if (win_loc == JG_PTR_HOST && fsize >= 3) {
    int longest = 0;
    for (int64_t i = 0; i < n_win; ++i) longest = std::max(longest, std::min(win_len[i], fsize));
    need = nt_ids ? longest : row_len(longest);
  }
  JG_REQUIRE(fsize >= 3 && l_pad >= need && l_pad >= 1, JG_ERR_INVALID,
             "encode: l_pad=%d is smaller than the %d %s the longest window yields (fsize %d)", l_pad,
             need, nt_ids ? "bases" : "codons", fsize);
  const uint8_t *d_bases = bases;
  if (bases_loc == JG_PTR_HOST) {
    void *p = nullptr;
    if (scratch_owner != nullptr) {
      const int rc = grow(&scratch_owner->d_bases_buf, &scratch_owner->d_bases_cap, std::max<int64_t>(n_bases, 1));
      if (rc != JG_OK) return rc;
      p = scratch_owner->d_bases_buf;
    } else {
      JG_HIP(hipMalloc(&p, (size_t)std::max<int64_t>(n_bases, 1)));
      to_free.push_back(p);
    }
    JG_HIP(hipMemcpyAsync(p, bases, (size_t)n_bases, hipMemcpyHostToDevice, s));
    d_bases = static_cast<const uint8_t *>(p);
    if (e->n_rec > 0) {                       // records attached: DUST on the uploaded copy, the encoder respects the case
      JG_REQUIRE(e->rec_end <= n_bases, JG_ERR_INVALID, "encode: the attached records end at %lld, beyond the %lld-byte base buffer",
                 (long long)e->rec_end, (long long)n_bases);
      const int rc = jg_launch_dust(static_cast<uint8_t *>(p), 0, n_bases, e->d_rec_off, e->n_rec, e->dust_window,
                                    e->dust_threshold, 0, n_bases, e->d_dust_cnt, s);
      if (rc != JG_OK) return rc;
      flags |= 1;
    }
  }
  const int64_t *d_start = win_start;
  const int32_t *d_len = win_len;
  if (win_loc == JG_PTR_HOST) {
    // validate on the host: every window must lie inside the base buffer
    for (int64_t i = 0; i < n_win; ++i)
      JG_REQUIRE(win_start[i] >= 0 && win_len[i] >= 0 && win_start[i] + win_len[i] <= n_bases,
                 JG_ERR_INVALID, "encode: window %lld [%lld, +%d) outside the %lld-byte base buffer",
                 (long long)i, (long long)win_start[i], win_len[i], (long long)n_bases);
    void *p = nullptr;
    if (scratch_owner != nullptr) {
      const int rc = grow(&scratch_owner->d_win, &scratch_owner->d_win_cap, n_win * 12);
      if (rc != JG_OK) return rc;
      p = scratch_owner->d_win;
    } else {
      JG_HIP(hipMalloc(&p, (size_t)n_win * 12));
      to_free.push_back(p);
    }
    JG_HIP(hipMemcpyAsync(p, win_start, (size_t)n_win * 8, hipMemcpyHostToDevice, s));
    JG_HIP(hipMemcpyAsync(static_cast<char *>(p) + n_win * 8, win_len, (size_t)n_win * 4,
                          hipMemcpyHostToDevice, s));
    d_start = static_cast<const int64_t *>(p);
    d_len = reinterpret_cast<const int32_t *>(static_cast<char *>(p) + n_win * 8);
  }
  JG_HIP(hipMemcpyAsync(d_lut, lut65, 65, hipMemcpyHostToDevice, s));
  return jg_launch_encode(d_bases, d_start, d_len, n_win, fsize, d_lut, flags, l_pad, d_ids,
                          d_counts, s);
}

extern "C" int jg_encode(jg_engine *e, const uint8_t *bases, int64_t n_bases, int bases_loc,
                         const int64_t *win_start, const int32_t *win_len, int win_loc,
                         int64_t n_win, int32_t fsize, const uint8_t *lut65, int32_t soft_mask,
                         int32_t l_pad, uint8_t *ids, int32_t *counts, int out_loc, void *stream) {
  JG_REQUIRE(e != nullptr && bases != nullptr && win_start != nullptr && win_len != nullptr &&
                 lut65 != nullptr && ids != nullptr && n_win >= 0,
             JG_ERR_INVALID, "jg_encode: bad arguments");
  if (n_win == 0) return JG_OK;
  JG_HIP(hipSetDevice(e->dev));
  hipStream_t s = pick_stream(e, stream);
  std::vector<void *> to_free;
  uint8_t *d_ids = ids;
  int32_t *d_counts = counts;
  const int64_t id_bytes = n_win * ((soft_mask & JG_ENC_NUCLEOTIDE) ? 2 : 6) * (int64_t)l_pad * ((soft_mask & JG_ENC_DICODON) ? 2 : 1);
  void *d_lut = nullptr;
  JG_HIP(hipMalloc(&d_lut, 80));
  to_free.push_back(d_lut);
  if (out_loc == JG_PTR_HOST) {
    void *p = nullptr;
    JG_HIP(hipMalloc(&p, (size_t)id_bytes));
    to_free.push_back(p);
    d_ids = static_cast<uint8_t *>(p);
    if (counts != nullptr) {
      JG_HIP(hipMalloc(&p, (size_t)n_win * 16));
      to_free.push_back(p);
      d_counts = static_cast<int32_t *>(p);
    }
  }
  int rc = encode_common(e, nullptr, bases, n_bases, bases_loc, win_start, win_len, win_loc, n_win,
                         fsize, lut65, soft_mask, l_pad, d_ids, d_counts,
                         static_cast<uint8_t *>(d_lut), to_free, s);
  if (rc == JG_OK && out_loc == JG_PTR_HOST) {
    hipError_t err = hipMemcpyAsync(ids, d_ids, (size_t)id_bytes, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess && counts != nullptr)
      err = hipMemcpyAsync(counts, d_counts, (size_t)n_win * 16, hipMemcpyDeviceToHost, s);
    if (err != hipSuccess) {
      jg_set_error("jg_encode: D2H copy -> %s", hipGetErrorString(err));
      rc = JG_ERR_HIP;
    }
  }
  if (!to_free.empty() || out_loc == JG_PTR_HOST) (void)hipStreamSynchronize(s);
  for (void *p : to_free) (void)hipFree(p);
  return rc;
}

// ---- streamed ingest -------------------------------------------------------------------------
// Host-resident bases larger than the engine's stream budget never exist on the device as a whole: the
// (start-sorted) window list is cut into groups whose base span fits the budget and whose window count is a whole
// number of forward passes.  The groups run as a two-deep pipeline that never drains the compute stream:
//   helper thread   span of group g+1: host -> pinned staging -> device buffer (g+1)%2 on the copy stream
//   compute stream  group g: window table (pinned) -> [DUST] -> encode -> forward passes -> outputs D2H into pinned
//                   staging g%2 -> event
//   calling thread  after ENQUEUEING group g it waits for group g-1's event, copies that group's rows from the pinned
//                   staging into the caller's arrays and publishes the progress (JG_STAT_WINDOWS_DONE): the rows of
//                   windows below that mark are final while the call is still running.
// Nothing in the loop synchronises the whole stream; buffers are recycled on events (device span: the encode that
// read it; pinned span: its H2D copy; pinned outputs: the calling thread's own copy-out).
static int stream_setup(jg_engine *e, int64_t span_cap, int64_t io_cap) {
  if (e->copy_stream == nullptr) JG_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    if (e->h2d_done[i] == nullptr) JG_HIP(hipEventCreateWithFlags(&e->h2d_done[i], hipEventDisableTiming));
    if (e->enc_done[i] == nullptr) JG_HIP(hipEventCreateWithFlags(&e->enc_done[i], hipEventDisableTiming));
    if (e->grp_done[i] == nullptr)
      JG_HIP(hipEventCreateWithFlags(&e->grp_done[i], hipEventDisableTiming | hipEventBlockingSync));
  }
  if (span_cap > e->pin_cap) {
    for (int i = 0; i < 2; ++i) {
      if (e->pin[i]) JG_HIP(hipHostFree(e->pin[i]));
      e->pin[i] = nullptr;
      JG_HIP(hipHostMalloc(&e->pin[i], (size_t)span_cap, hipHostMallocDefault));
    }
    e->pin_cap = span_cap;
  }
  if (span_cap > e->dbase_cap) {
    for (int i = 0; i < 2; ++i) {
      if (e->dbase[i]) JG_HIP(hipFree(e->dbase[i]));
      e->dbase[i] = nullptr;
      JG_HIP(hipMalloc(&e->dbase[i], (size_t)span_cap));
    }
    e->dbase_cap = span_cap;
  }
  if (io_cap > e->pin_io_cap) {
    for (int i = 0; i < 2; ++i) {
      if (e->pin_io[i]) JG_HIP(hipHostFree(e->pin_io[i]));
      e->pin_io[i] = nullptr;
      JG_HIP(hipHostMalloc(&e->pin_io[i], (size_t)io_cap, hipHostMallocDefault));
    }
    e->pin_io_cap = io_cap;
  }
  return JG_OK;
}

struct StreamGroup {
  int64_t w0, w1;      // windows [w0, w1)
  int64_t b0, b1;      // base span [b0, b1) they touch
};

// Groups of a start-sorted window list: base span <= budget; a group that holds at least one whole forward pass is cut
// back to a multiple of `chunk` windows, so that only a call's last pass is ragged.
static void stream_groups(const int64_t *win_start, const int32_t *win_len, int64_t n_win, int64_t budget, int64_t chunk,
                          std::vector<StreamGroup> &groups) {
  int64_t i = 0;
  while (i < n_win) {
    // ramp: the first span is an eighth of the budget and the second a half, so that the compute stream has work after a
    // millisecond of staging instead of after a whole span (nothing hides the first span's copy, upload and DUST pass)
    const size_t gi = groups.size();
    const int64_t cap = gi == 0 ? std::max<int64_t>(budget / 8, 4096) : (gi == 1 ? std::max<int64_t>(budget / 2, 4096) : budget);
    StreamGroup g{i, i, win_start[i], win_start[i] + win_len[i]};
    int64_t j = i + 1;
    for (; j < n_win; ++j) {
      const int64_t b1 = std::max(g.b1, win_start[j] + win_len[j]);
      if (b1 - g.b0 > cap) break;
      g.b1 = b1;
    }
    if (j < n_win && j - i >= chunk && (j - i) % chunk != 0) {
      j = i + (j - i) / chunk * chunk;
      g.b1 = g.b0;
      for (int64_t q = i; q < j; ++q) g.b1 = std::max(g.b1, win_start[q] + win_len[q]);
    }
    g.w1 = j;
    groups.push_back(g);
    i = j;
  }
}

static int predict_streamed(jg_model *m, const uint8_t *bases, int64_t n_bases, const int64_t *win_start,
                            const int32_t *win_len, int64_t n_win, int32_t fsize, const uint8_t *lut65,
                            int32_t flags, int32_t l_pad, float *prediction, float *reliability,
                            float *embedding, float *nmd, int32_t *counts, int out_loc, int32_t chunk,
                            hipStream_t s) {
  jg_engine *e = m->e;
  const int64_t budget = e->stream_bytes;
  const int fchunk = jg_effective_chunk(m, chunk, l_pad, n_win);
  JG_REQUIRE((int64_t)fchunk * 6 <= 0x7fffffff / 8, JG_ERR_INVALID, "chunk too large");
  std::vector<StreamGroup> groups;
  stream_groups(win_start, win_len, n_win, budget, fchunk, groups);
  int64_t span_cap = 0, win_cap = 0;
  for (const StreamGroup &q : groups) {
    span_cap = std::max(span_cap, q.b1 - q.b0);
    win_cap = std::max(win_cap, q.w1 - q.w0);
  }
  // with records attached (jg_engine_set_dust) every span is staged with 64 bases of context either side and
  // soft-masked on the device before it is encoded: an interval that touches a window starts or ends < 64 bases outside it
  const bool dust = e->n_rec > 0;
  const int64_t ctx = dust ? 64 : 0;
  if (dust) {
    JG_REQUIRE(e->rec_end <= n_bases, JG_ERR_INVALID, "encode: the attached records end at %lld, beyond the %lld-byte base buffer",
               (long long)e->rec_end, (long long)n_bases);
    flags |= 1;
  }
  span_cap = (span_cap + 2 * ctx + 4095) / 4096 * 4096;
  // pinned staging per parity: [window starts i64][window lengths i32][outputs f32 ...][counts i32 x 4][range-guard flag]
  const bool host_out = out_loc == JG_PTR_HOST;
  const int w_pred = jg_model_vec_width(m, 0), w_rel = jg_model_vec_width(m, 1);
  const int w_emb = jg_model_vec_width(m, 2), w_nmd = jg_model_vec_width(m, 3);
  float *user[4] = {prediction, reliability, embedding, nmd};
  const int width[4] = {w_pred, w_rel, w_emb, w_nmd};
  int64_t off_out[4] = {0, 0, 0, 0};
  int64_t io = (win_cap * 12 + 63) / 64 * 64;
  for (int k = 0; k < 4; ++k) {
    off_out[k] = io;
    if (host_out && user[k] != nullptr && width[k] > 0) io += (win_cap * width[k] * 4 + 63) / 64 * 64;
  }
  const int64_t off_counts = io;
  if (host_out && counts != nullptr) io += win_cap * 16;
  const int64_t off_flag = io;
  io += 64;
  int rc = stream_setup(e, std::max<int64_t>(span_cap, 4096), (io + 4095) / 4096 * 4096);
  if (rc != JG_OK) return rc;
  if ((rc = grow(&m->d_ids, &m->d_ids_cap, win_cap * 6 * (int64_t)l_pad * m->id_bytes)) != JG_OK) return rc;
  if ((rc = grow(&m->d_win, &m->d_win_cap, win_cap * 12)) != JG_OK) return rc;
  if (counts != nullptr && host_out)
    if ((rc = grow(&m->d_counts, &m->d_counts_cap, win_cap * 16)) != JG_OK) return rc;
  std::vector<OpShape> shp;                       // (one shape walk for the whole call: every group runs at l_pad)
  if ((rc = jg_shape_walk(m, l_pad, shp)) != JG_OK || (rc = jg_ensure_workspace(m, (int64_t)fchunk * m->strands, l_pad, shp)) != JG_OK) return rc;
  JG_HIP(hipMemcpyAsync(m->d_lut, lut65, 65, hipMemcpyHostToDevice, s));
  JG_HIP(hipStreamSynchronize(s));               // (lut65 is the caller's pageable memory; nothing else waits in the loop)
  e->streamed_groups = (int64_t)groups.size();
  e->streamed_bytes = 0;
  e->peak_dev_bases = 2 * e->dbase_cap;

  bool span_used[2] = {false, false};            // parity b's device span / pinned span have been used in this pipeline run
  auto stage = [&](size_t gi) -> int {           // host span -> pinned -> device buffer gi % 2 (copy stream)
    const StreamGroup &g = groups[gi];
    const int b = (int)(gi & 1);
    JG_HIP(hipSetDevice(e->dev));
    const int64_t h0 = std::max<int64_t>(0, g.b0 - ctx), h1 = std::min(n_bases, g.b1 + ctx);
    if (span_used[b]) JG_HIP(hipEventSynchronize(e->h2d_done[b]));                 // the pinned span's last copy has left it
    memcpy(e->pin[b], bases + h0, (size_t)(h1 - h0));
    if (span_used[b]) JG_HIP(hipStreamWaitEvent(e->copy_stream, e->enc_done[b], 0));   // the device span's last reader is done
    JG_HIP(hipMemcpyAsync(e->dbase[b], e->pin[b], (size_t)(h1 - h0), hipMemcpyHostToDevice, e->copy_stream));
    if (dust && e->dust_on_copy) {
      // DUST on the copy stream, behind the span's upload: a vector / LDS kernel that shares the CUs with the matrix-core
      // convolutions of the previous group instead of standing in front of this group's encoder on the compute stream
      const int drc = jg_launch_dust(static_cast<uint8_t *>(e->dbase[b]), h0, h1 - h0, e->d_rec_off, e->n_rec, e->dust_window,
                                     e->dust_threshold, g.b0, g.b1, e->d_dust_cnt, e->copy_stream);
      if (drc != JG_OK) return drc;
    }
    JG_HIP(hipEventRecord(e->h2d_done[b], e->copy_stream));
    span_used[b] = true;
    e->streamed_bytes += g.b1 - g.b0;
    return JG_OK;
  };
  auto enqueue = [&](size_t gi) -> int {         // everything group gi needs of the compute stream
    const StreamGroup &g = groups[gi];
    const int b = (int)(gi & 1);
    const int64_t nw = g.w1 - g.w0;
    char *io_b = static_cast<char *>(e->pin_io[b]);
    int64_t *p_start = reinterpret_cast<int64_t *>(io_b);
    int32_t *p_len = reinterpret_cast<int32_t *>(io_b + win_cap * 8);
    const int64_t h0 = std::max<int64_t>(0, g.b0 - ctx);                                       // start of the staged span
    for (int64_t i = 0; i < nw; ++i) p_start[i] = win_start[g.w0 + i] - h0;
    memcpy(p_len, win_len + g.w0, (size_t)nw * 4);
    char *dw = static_cast<char *>(m->d_win);
    JG_HIP(hipMemcpyAsync(dw, io_b, (size_t)(win_cap * 8 + nw * 4), hipMemcpyHostToDevice, s));
    JG_HIP(hipStreamWaitEvent(s, e->h2d_done[b], 0));          // (uploaded and - JG_OPT_DUST_ON_COPY_STREAM - soft-masked)
    if (dust && !e->dust_on_copy) {
      const int64_t h1 = std::min(n_bases, g.b1 + ctx);
      const int drc = jg_launch_dust(static_cast<uint8_t *>(e->dbase[b]), h0, h1 - h0, e->d_rec_off, e->n_rec, e->dust_window,
                                     e->dust_threshold, g.b0, g.b1, e->d_dust_cnt, s);
      if (drc != JG_OK) return drc;
    }
    int32_t *d_counts = counts == nullptr ? nullptr : (host_out ? m->d_counts : counts + g.w0 * 4);
    int erc = jg_launch_encode(static_cast<const uint8_t *>(e->dbase[b]), reinterpret_cast<const int64_t *>(dw),
                               reinterpret_cast<const int32_t *>(dw + win_cap * 8), nw, fsize, m->d_lut, flags, l_pad,
                               m->d_ids, d_counts, s);
    if (erc != JG_OK) return erc;
    JG_HIP(hipEventRecord(e->enc_done[b], s));
    float *dst[4];
    for (int k = 0; k < 4; ++k)
      dst[k] = user[k] == nullptr ? nullptr
                                  : (host_out ? reinterpret_cast<float *>(io_b + off_out[k]) : user[k] + g.w0 * width[k]);
    // (JG_OPT_POISON_WORKSPACE: every pass fills the workspace on `s` first - behind the previous group's copies into its
    // pinned staging, which are queued on `s` as well; grp_done guards the staging, not the workspace)
    erc = jg_forward_chunks(m, shp, m->d_ids, nw, l_pad, dst[0], dst[1], dst[2], dst[3], out_loc, fchunk, s);
    if (erc != JG_OK) return erc;
    if (counts != nullptr && host_out)
      JG_HIP(hipMemcpyAsync(io_b + off_counts, d_counts, (size_t)nw * 16, hipMemcpyDeviceToHost, s));
    if (m->precision == 1)
      JG_HIP(hipMemcpyAsync(io_b + off_flag, m->d_overflow, sizeof(int), hipMemcpyDeviceToHost, s));
    JG_HIP(hipEventRecord(e->grp_done[b], s));
    return JG_OK;
  };
  // wait for group gi, hand its rows to the caller, publish the progress; *overflow: the f16 range guard tripped in it
  auto finalize = [&](size_t gi, bool *overflow) -> int {
    const StreamGroup &g = groups[gi];
    const int b = (int)(gi & 1);
    const int64_t nw = g.w1 - g.w0;
    JG_HIP(hipEventSynchronize(e->grp_done[b]));
    const char *io_b = static_cast<const char *>(e->pin_io[b]);
    if (m->precision == 1 && *reinterpret_cast<const int *>(io_b + off_flag) != 0) {
      *overflow = true;
      return JG_OK;
    }
    if (host_out) {
      for (int k = 0; k < 4; ++k)
        if (user[k] != nullptr && width[k] > 0)
          memcpy(user[k] + g.w0 * width[k], io_b + off_out[k], (size_t)nw * width[k] * 4);
      if (counts != nullptr) memcpy(counts + g.w0 * 4, io_b + off_counts, (size_t)nw * 16);
    }
    e->windows_done.store(g.w1, std::memory_order_release);
    return JG_OK;
  };

  size_t first = 0;
  while (first < groups.size()) {
    span_used[0] = span_used[1] = false;
    if ((rc = stage(first)) != JG_OK) return rc;
    bool overflow = false;
    size_t redo = groups.size();
    for (size_t gi = first; gi < groups.size() && !overflow; ++gi) {
      // the next group's span is staged by a helper thread while this group is enqueued and the previous one handed over
      int stage_rc = JG_OK;
      std::string stage_err;
      std::thread stager;
      if (gi + 1 < groups.size())
        stager = std::thread([&, gi]() {
          stage_rc = stage(gi + 1);
          if (stage_rc != JG_OK) stage_err = jg_last_error();
        });
      struct Joiner {
        std::thread &t;
        ~Joiner() { if (t.joinable()) t.join(); }
      } joiner{stager};
      if ((rc = enqueue(gi)) != JG_OK) return rc;
      if (gi > first) {
        if ((rc = finalize(gi - 1, &overflow)) != JG_OK) return rc;
        if (overflow) redo = gi - 1;
      }
      if (stager.joinable()) stager.join();
      if (stage_rc != JG_OK) {
        jg_set_error("%s", stage_err.c_str());
        return stage_rc;
      }
    }
    if (!overflow) {
      if ((rc = finalize(groups.size() - 1, &overflow)) != JG_OK) return rc;
      if (overflow) redo = groups.size() - 1;
    }
    if (!overflow) break;
    // split-f16 range guard: an activation beyond the f16 range poisons the fast path - drain the pipeline, fall back to the
    // exact-f32 kernels for the group that tripped it, for every later group and for every later call of the model
    JG_HIP(hipStreamSynchronize(s));
    JG_HIP(hipStreamSynchronize(e->copy_stream));
    JG_HIP(hipMemsetAsync(m->d_overflow, 0, sizeof(int), s));
    m->precision = 0;
    m->f16_reason = "an activation left the f16 range at run time";
    if ((rc = jg_ensure_workspace(m, (int64_t)fchunk * m->strands, l_pad, shp)) != JG_OK) return rc;
    first = redo;
  }
  JG_HIP(hipStreamSynchronize(s));
  return JG_OK;
}

extern "C" int jg_predict_windows(jg_model *m, const uint8_t *bases, int64_t n_bases, int bases_loc,
                                  const int64_t *win_start, const int32_t *win_len, int win_loc,
                                  int64_t n_win, int32_t fsize, const uint8_t *lut65,
                                  int32_t soft_mask, int32_t l_pad, float *prediction,
                                  float *reliability, float *embedding, float *nmd, int32_t *counts,
                                  int out_loc, int32_t chunk, void *stream) {
  JG_REQUIRE(m != nullptr && bases != nullptr && win_start != nullptr && win_len != nullptr &&
                 lut65 != nullptr && n_win >= 0,
             JG_ERR_INVALID, "jg_predict_windows: bad arguments");
  JG_REQUIRE(m->tap_op < 0, JG_ERR_UNSUPPORTED, "jg_predict_windows: a tap is set (op %d): taps are read through jg_forward only",
             m->tap_op);
  jg_engine *e = m->e;
  e->windows_done.store(0, std::memory_order_release);       // (also for an empty call: a poller must not see the previous call's mark)
  if (n_win == 0) return JG_OK;
  JG_HIP(hipSetDevice(e->dev));
  hipStream_t s = pick_stream(e, stream);
  e->streamed_groups = 0;
  e->streamed_bytes = 0;
  e->peak_dev_bases = bases_loc == JG_PTR_HOST ? n_bases : 0;
  e->windows_done.store(0, std::memory_order_release);
  if (m->strands > 1) soft_mask |= JG_ENC_NUCLEOTIDE;       // a two-strand model reads nucleotide ids (n_win, 2, l_pad)
  if (m->id_bytes == 2) soft_mask |= JG_ENC_DICODON;        // a dicodon model reads 16-bit ids of codon pairs
  if (bases_loc == JG_PTR_HOST && win_loc == JG_PTR_HOST && n_bases > e->stream_bytes) {
    // streamed ingest needs a start-sorted window list (the fragmenter's FASTA order is) inside the buffer
    bool sorted = true;
    int longest = 0;
    for (int64_t i = 0; i < n_win; ++i) {
      JG_REQUIRE(win_start[i] >= 0 && win_len[i] >= 0 && win_start[i] + win_len[i] <= n_bases, JG_ERR_INVALID,
                 "encode: window %lld [%lld, +%d) outside the %lld-byte base buffer", (long long)i,
                 (long long)win_start[i], win_len[i], (long long)n_bases);
      sorted &= i == 0 || win_start[i] >= win_start[i - 1];
      longest = std::max(longest, std::min(win_len[i], fsize));
    }
    if (sorted) {
      const int off3 = (fsize % 3 == 0) ? -2 : ((fsize % 3 == 1) ? -1 : 0);
      const int usable = longest - 5 + off3, usable6 = longest - 8 + off3;
      const int need = m->strands > 1 ? longest : m->id_bytes == 2 ? (usable6 > 0 ? (usable6 + 5) / 6 : 0)
                                                                   : (usable > 0 ? (usable + 2) / 3 : 0);
      JG_REQUIRE(fsize >= 3 && l_pad >= need && l_pad >= 1, JG_ERR_INVALID,
                 "encode: l_pad=%d is smaller than the %d %s the longest window yields (fsize %d)", l_pad, need,
                 m->strands > 1 ? "bases" : "codons", fsize);
      return predict_streamed(m, bases, n_bases, win_start, win_len, n_win, fsize, lut65, soft_mask, l_pad,
                              prediction, reliability, embedding, nmd, counts, out_loc, chunk, s);
    }
  }
  std::vector<void *> to_free;
  int rc = grow(&m->d_ids, &m->d_ids_cap, n_win * 6 * (int64_t)l_pad * m->id_bytes);
  if (rc != JG_OK) return rc;
  int32_t *d_counts = counts;
  if (counts != nullptr && out_loc == JG_PTR_HOST) {
    rc = grow(&m->d_counts, &m->d_counts_cap, n_win * 16);
    if (rc != JG_OK) return rc;
    d_counts = m->d_counts;
  }
  rc = encode_common(e, m, bases, n_bases, bases_loc, win_start, win_len, win_loc, n_win, fsize,
                     lut65, soft_mask, l_pad, m->d_ids, d_counts, m->d_lut, to_free, s);
  if (rc == JG_OK)
    rc = jg_forward_device_ids(m, m->d_ids, n_win, l_pad, prediction, reliability, embedding, nmd,
                            out_loc, chunk, s);
  if (rc == JG_OK && counts != nullptr && out_loc == JG_PTR_HOST) {
    hipError_t err = hipMemcpyAsync(counts, d_counts, (size_t)n_win * 16, hipMemcpyDeviceToHost, s);
    if (err != hipSuccess) {
      jg_set_error("jg_predict_windows: counts D2H -> %s", hipGetErrorString(err));
      rc = JG_ERR_HIP;
    }
  }
  if (!to_free.empty() || out_loc == JG_PTR_HOST) (void)hipStreamSynchronize(s);
  for (void *p : to_free) (void)hipFree(p);
  if (rc == JG_OK && out_loc == JG_PTR_HOST) e->windows_done.store(n_win, std::memory_order_release);
  return rc;
}
