// C-ABI of libjaeger_hip.so (see include/jaeger_hip.h), engine part: create / destroy, options, statistics, device memory,
// timers and the read-out of the profiling brackets (jg_run.hip opens them).  Host logic only.
#include <stdarg.h>
#include <stdio.h>

#include "jg_host.h"

static thread_local char g_err[1024] = "";

void jg_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *jg_last_error(void) { return g_err; }
extern "C" int jg_abi_version(void) { return JG_ABI_VERSION; }
extern "C" int jg_localattn_tile(void) { return JG_LOCALATTN_TILE; }
extern "C" int jg_lengthattn_tile(void) { return JG_LENGTHATTN_TILE; }
extern "C" int jg_lengthattn_chunk(void) { return JG_LENGTHATTN_CHUNK; }
extern "C" int jg_hyena_tile(void) { return JG_HYENA_TILE; }
extern "C" int jg_hyena_chunk(void) { return JG_HYENA_CHUNK; }
extern "C" int jg_bilstm_rows(void) { return JG_BILSTM_ROWS; }
extern "C" int jg_bilstm_steps(void) { return JG_BILSTM_STEPS; }
extern "C" int jg_msconv_tile(void) { return JG_MSCONV_TILE; }
extern "C" int jg_sizeof(int which) {
  return which == 0 ? (int)sizeof(jg_op) : (which == 1 ? (int)sizeof(jg_stage) : -1);
}

extern "C" int jg_engine_create(int device_id, jg_engine **out) {
  JG_REQUIRE(out != nullptr, JG_ERR_INVALID, "jg_engine_create: out is NULL");
  int n_dev = 0;
  JG_HIP(hipGetDeviceCount(&n_dev));
  JG_REQUIRE(device_id >= 0 && device_id < n_dev, JG_ERR_INVALID,
             "jg_engine_create: device %d not present (%d visible)", device_id, n_dev);
  JG_HIP(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  JG_HIP(hipGetDeviceProperties(&prop, device_id));
  JG_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, JG_ERR_UNSUPPORTED,
             "jg_engine_create: device %d is %s; this library targets gfx950 (MI355X) only",
             device_id, prop.gcnArchName);
  jg_engine *e = new jg_engine();
  e->dev = device_id;
  e->n_cu = prop.multiProcessorCount;
  JG_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  JG_HIP(hipEventCreate(&e->t0));
  JG_HIP(hipEventCreate(&e->t1));
  *out = e;
  return JG_OK;
}

extern "C" int jg_engine_destroy(jg_engine *e) {
  if (e == nullptr) return JG_OK;
  (void)hipSetDevice(e->dev);
  (void)hipStreamSynchronize(e->stream);
  for (auto &p : e->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto ev : e->pool) (void)hipEventDestroy(ev);
  (void)hipEventDestroy(e->t0);
  (void)hipEventDestroy(e->t1);
  for (int i = 0; i < 2; ++i) {
    if (e->pin[i]) (void)hipHostFree(e->pin[i]);
    if (e->dbase[i]) (void)hipFree(e->dbase[i]);
    if (e->h2d_done[i]) (void)hipEventDestroy(e->h2d_done[i]);
    if (e->enc_done[i]) (void)hipEventDestroy(e->enc_done[i]);
    if (e->grp_done[i]) (void)hipEventDestroy(e->grp_done[i]);
    if (e->pin_io[i]) (void)hipHostFree(e->pin_io[i]);
  }
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->d_rec_off) (void)hipFree(e->d_rec_off);
  if (e->d_dust_cnt) (void)hipFree(e->d_dust_cnt);
  (void)hipStreamDestroy(e->stream);
  delete e;
  return JG_OK;
}

extern "C" int jg_engine_sync(jg_engine *e) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_engine_sync: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  JG_HIP(hipStreamSynchronize(e->stream));
  return JG_OK;
}

extern "C" int jg_engine_set_option(jg_engine *e, int key, int64_t value) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_engine_set_option: NULL engine");
  switch (key) {
    case JG_OPT_STREAM_BYTES:
      JG_REQUIRE(value >= 4096, JG_ERR_INVALID, "jg_engine_set_option: stream budget %lld < 4096 bytes", (long long)value);
      e->stream_bytes = value;
      return JG_OK;
    case JG_OPT_CONV_PC:
      JG_REQUIRE(value >= 0 && value <= 2, JG_ERR_INVALID, "jg_engine_set_option: JG_OPT_CONV_PC takes 0, 1 or 2, got %lld", (long long)value);
#ifndef JG_EXPERIMENT
      JG_REQUIRE(value == 0, JG_ERR_UNSUPPORTED, "jg_engine_set_option: JG_OPT_CONV_PC = %lld needs the experiment build (make -C jaeger_amd/csrc "
                 "exp; JAEGER_HIP_LIB=jaeger_amd/libjaeger_hip_exp.so): the producer / consumer kernels are not in the shipped library",
                 (long long)value);
#endif
      e->conv_pc = (int)value;
      return JG_OK;
    case JG_OPT_TERMINI_EXACT:
      e->termini_exact = value != 0;
      return JG_OK;
    case JG_OPT_TERMINI_REPORT_MIN:
      JG_REQUIRE(value == 0 || (value >= 2 && value <= 15), JG_ERR_INVALID,
                 "jg_engine_set_option: JG_OPT_TERMINI_REPORT_MIN = %lld (0, or 2 .. 15 columns)", (long long)value);
      e->termini_report_min = (int)value;
      return JG_OK;
    case JG_OPT_DUST_ON_COPY_STREAM:
      e->dust_on_copy = value != 0;
      return JG_OK;
    case JG_OPT_TABLE_NET_LDS:
      e->tab_lds_only = value != 0;
      return JG_OK;
    case JG_OPT_FUSE_RESBLOCK:
      e->fuse_resblock = value != 0;
      return JG_OK;
    case JG_OPT_POISON_WORKSPACE:
      JG_REQUIRE(value >= -1 && value <= 255, JG_ERR_INVALID, "jg_engine_set_option: JG_OPT_POISON_WORKSPACE takes -1 (off) or a byte 0 .. 255, got %lld",
                 (long long)value);
      e->poison = (int)value;
      return JG_OK;
    case JG_OPT_RESET_PROGRESS:
      e->windows_done.store(0, std::memory_order_release);
      return JG_OK;
    case JG_OPT_STREAM_PRIORITY: {
      JG_REQUIRE(value == 0 || value == 1, JG_ERR_INVALID, "jg_engine_set_option: JG_OPT_STREAM_PRIORITY takes 0 or 1, got %lld",
                 (long long)value);
      JG_HIP(hipSetDevice(e->dev));
      JG_HIP(hipStreamSynchronize(e->stream));                   // (an idle engine: nothing is waited for)
      int least = 0, greatest = 0;                               // numerically lower = more urgent
      JG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      hipStream_t fresh = nullptr;
      JG_HIP(hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, value ? greatest : least));
      (void)hipStreamDestroy(e->stream);
      e->stream = fresh;
      return JG_OK;
    }
    default:
      jg_set_error("jg_engine_set_option: unknown key %d", key);
      return JG_ERR_INVALID;
  }
}

extern "C" int64_t jg_engine_get_stat(const jg_engine *e, int key) {
  if (e == nullptr) return -1;
  switch (key) {
    case JG_STAT_STREAM_GROUPS: return e->streamed_groups;
    case JG_STAT_STREAM_BYTES: return e->streamed_bytes;
    case JG_STAT_PEAK_DEVICE_BASES: return e->peak_dev_bases;
    case JG_STAT_WINDOWS_DONE: return e->windows_done.load(std::memory_order_acquire);
    case JG_STAT_DUST_MASKED: {          // bases the device DUST lower-cased since the records were attached (syncs)
      if (e->d_dust_cnt == nullptr) return 0;
      unsigned long long h = 0;
      if (hipSetDevice(e->dev) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
          hipMemcpy(&h, e->d_dust_cnt, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
      return (int64_t)h;
    }
    default: return -1;
  }
}

// Attach the record table of the host base buffer the following jg_predict_windows / jg_encode calls will be given:
// their uploaded copy of the bases is then soft-masked on the device (symmetric DUST, jg_dust.hip) before it is
// encoded, and the encoder respects the case.  n_records = 0 (or rec_off NULL) detaches.
extern "C" int jg_engine_set_dust(jg_engine *e, const int64_t *rec_off, int64_t n_records, int32_t window,
                                  int32_t threshold) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_engine_set_dust: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  if (rec_off == nullptr || n_records <= 0) {
    e->n_rec = 0;
    return JG_OK;
  }
  JG_REQUIRE(window >= 4 && window <= 64 && threshold > 0, JG_ERR_UNSUPPORTED,
             "jg_engine_set_dust: window %d outside 4..64 (mask on the host with jg_dust_mask)", window);
  for (int64_t r = 0; r < n_records; ++r)
    JG_REQUIRE(rec_off[r] >= 0 && rec_off[r + 1] >= rec_off[r], JG_ERR_INVALID, "jg_engine_set_dust: record %lld has a negative length",
               (long long)r);
  JG_HIP(hipStreamSynchronize(e->stream));            // (a previous call may still read the old table)
  if (n_records + 1 > e->rec_cap) {
    if (e->d_rec_off) JG_HIP(hipFree(e->d_rec_off));
    e->d_rec_off = nullptr;
    JG_HIP(hipMalloc(reinterpret_cast<void **>(&e->d_rec_off), (size_t)(n_records + 1) * sizeof(int64_t)));
    e->rec_cap = n_records + 1;
  }
  if (e->d_dust_cnt == nullptr) JG_HIP(hipMalloc(reinterpret_cast<void **>(&e->d_dust_cnt), sizeof(unsigned long long)));
  JG_HIP(hipMemcpy(e->d_rec_off, rec_off, (size_t)(n_records + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  JG_HIP(hipMemset(e->d_dust_cnt, 0, sizeof(unsigned long long)));
  e->n_rec = n_records;
  e->rec_end = rec_off[n_records];
  e->dust_window = window;
  e->dust_threshold = threshold;
  return JG_OK;
}

extern "C" int jg_dev_alloc(jg_engine *e, int64_t bytes, void **out) {
  JG_REQUIRE(e != nullptr && out != nullptr && bytes >= 0, JG_ERR_INVALID, "jg_dev_alloc: bad args");
  JG_HIP(hipSetDevice(e->dev));
  *out = nullptr;
  if (bytes == 0) return JG_OK;
  hipError_t err = hipMalloc(out, (size_t)bytes);
  if (err != hipSuccess) {
    jg_set_error("jg_dev_alloc: hipMalloc(%lld) -> %s", (long long)bytes, hipGetErrorString(err));
    return JG_ERR_NOMEM;
  }
  return JG_OK;
}

extern "C" int jg_dev_free(jg_engine *e, void *p) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_dev_free: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  if (p != nullptr) JG_HIP(hipFree(p));
  return JG_OK;
}

extern "C" int jg_memcpy_h2d(jg_engine *e, void *dst, const void *src, int64_t bytes) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_memcpy_h2d: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  if (bytes > 0) {
    JG_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, e->stream));
    JG_HIP(hipStreamSynchronize(e->stream));
  }
  return JG_OK;
}

extern "C" int jg_memcpy_d2h(jg_engine *e, void *dst, const void *src, int64_t bytes) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_memcpy_d2h: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  if (bytes > 0) {
    JG_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, e->stream));
    JG_HIP(hipStreamSynchronize(e->stream));
  }
  return JG_OK;
}

extern "C" int jg_timer_start(jg_engine *e, void *stream) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_timer_start: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  JG_HIP(hipEventRecord(e->t0, pick_stream(e, stream)));
  return JG_OK;
}

extern "C" int jg_timer_stop_ms(jg_engine *e, void *stream, float *ms) {
  JG_REQUIRE(e != nullptr && ms != nullptr, JG_ERR_INVALID, "jg_timer_stop_ms: bad args");
  JG_HIP(hipSetDevice(e->dev));
  JG_HIP(hipEventRecord(e->t1, pick_stream(e, stream)));
  JG_HIP(hipEventSynchronize(e->t1));
  JG_HIP(hipEventElapsedTime(ms, e->t0, e->t1));
  return JG_OK;
}

extern "C" int jg_profile_enable(jg_engine *e, int on) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_profile_enable: NULL engine");
  e->profile = on != 0;
  e->conv_ms = 0.0;
  e->conv_flops = 0.0;
  e->conv_launches = 0;
  for (int i = 0; i < JG_PROF_CLASSES; ++i) { e->cls_ms[i] = 0.0; e->cls_flops[i] = 0.0; e->cls_launches[i] = 0; }
  return JG_OK;
}

static int drain_profile(jg_engine *e) {
  for (auto &p : e->pending) {
    JG_HIP(hipEventSynchronize(p.b));
    float ms = 0.f;
    JG_HIP(hipEventElapsedTime(&ms, p.a, p.b));
    e->conv_ms += ms;
    e->conv_flops += p.flops;
    e->conv_launches += 1;
    const int cls = p.cls >= 0 && p.cls < JG_PROF_CLASSES ? p.cls : 0;
    e->cls_ms[cls] += ms;
    e->cls_flops[cls] += p.flops;
    e->cls_launches[cls] += 1;
    e->pool.push_back(p.a);
    e->pool.push_back(p.b);
  }
  e->pending.clear();
  return JG_OK;
}

extern "C" int jg_profile_read(jg_engine *e, double *conv_ms, int64_t *conv_launches,
                               double *conv_flops) {
  JG_REQUIRE(e != nullptr, JG_ERR_INVALID, "jg_profile_read: NULL engine");
  JG_HIP(hipSetDevice(e->dev));
  int rc = drain_profile(e);
  if (rc != JG_OK) return rc;
  if (conv_ms) *conv_ms = e->conv_ms;
  if (conv_launches) *conv_launches = e->conv_launches;
  if (conv_flops) *conv_flops = e->conv_flops;
  return JG_OK;
}

extern "C" int jg_profile_read_class(jg_engine *e, int cls, double *ms, int64_t *launches, double *flops) {
  JG_REQUIRE(e != nullptr && cls >= 0 && cls < JG_PROF_CLASSES, JG_ERR_INVALID, "jg_profile_read_class: bad arguments");
  JG_HIP(hipSetDevice(e->dev));
  int rc = drain_profile(e);
  if (rc != JG_OK) return rc;
  if (ms) *ms = e->cls_ms[cls];
  if (launches) *launches = e->cls_launches[cls];
  if (flops) *flops = e->cls_flops[cls];
  return JG_OK;
}
