// Host side of libjaeger_hip.so, shared by jg_engine / jg_model / jg_prepare / jg_run / jg_predict.hip: the two tables
// every other piece reads - the shape record of each op at a row length, and where each op runs - and the few functions
// that cross the files - and the device-buffer / bucketing helpers of the host halves of jg_termini / jg_alignpairs.hip.  No
// kernel uses this header.
#pragma once
#include <string.h>

#include <algorithm>

#include "jg_common.h"
#include "jg_small.h"
#include "jg_resblock64.h"
#include "jg_vecmax.h"
#include "jg_frameattn.h"
#include "jg_localattn.h"
#include "jg_lengthattn.h"
#include "jg_hyena.h"
#include "jg_bilstm.h"
#include "jg_msconv.h"
#include "jg_poolvec.h"

#pragma GCC visibility push(hidden)
// ---- shapes: jg_shape_walk (jg_model.hip) is the only place that computes them -------------------------------------
struct Shape {
  int frames = 0, L = 0, C = 0;
};
struct OpShape {                // op i at l positions per row
  Shape in, out;                // the tensor in in_buf (ids: (id_frames, l, cin)) and the one written (frames 0: none)
  int L_out = 0, pad_left = 0;  // CONV / MASK geometry (MAXPOOL1D: L_out)
  int m_in = 0, m_out = 0;      // MASK / EMBED: positions per frame of the mask read and written
  int vec_need = 0;             // floats of out_vec this op needs (vec_off + its width)
  int64_t scratch = 0;          // HYENA: floats of the projection scratch per window
  Shape cvt[3];                 // the tensors converted in front of the op (ConvHPrep::cvt_slot), as they are then
};
int jg_shape_walk(const jg_model *m, int l, std::vector<OpShape> &shp);
int jg_ensure_workspace(jg_model *m, int64_t chunk, int l, const std::vector<OpShape> &shp);

// ---- placement: jg_place_op (jg_run.hip) is the only place that decides it -----------------------------------------
enum Place {
  PL_SMALL_SKIP,   // computed inside the small-window kernel: no launch
  PL_SMALL_NMD,    // NMD_FINAL that finishes a tap the small-window kernel accumulated
  PL_SMALL_POOL,   // POOL that finishes the small-window kernel's channel sums
  PL_TAB_CONV,     // table net: conv + pool in this op's launch
  PL_TAB_POOL,     // ... its pool: no launch
  PL_RB_CONV1,     // conv1 of a fused residual block: computed by conv2's launch
  PL_RB32,         // conv2 of a fused residual block: jg_resblock.hip
  PL_RB64,         // ... jg_resblock64.hip
  PL_CONV_F16,     // split-f16 conv
  PL_CONV_F32,     // exact-f32 conv
  PL_POOL_FUSED,   // POOL finished from the partials its split-f16 conv left
  PL_MIXER,        // a row mixer (below): launch_mixer
  PL_ORDINARY,     // the op's own kernel
};
struct PlaceCtx {  // what placement depends on besides the model
  int prec;        // 0 exact f32, 1 split-f16
  bool fuse_rb;    // JG_OPT_FUSE_RESBLOCK
  bool small, tab; // rows of this length fit the small-window kernel / the table net (false without a row length)
};
// of a run at l positions (shp = its shape walk); shp == nullptr: no row length, the layer-by-layer placement
PlaceCtx jg_place_ctx(const jg_model *m, const std::vector<OpShape> *shp, int l);
// the layer-by-layer placement in split-f16 mode under default options: what describe() and the statistics report
static inline PlaceCtx jg_place_nominal() { return PlaceCtx{1, true, false, false}; }
Place jg_place_op(const jg_model *m, size_t i, const PlaceCtx &c);
static inline bool jg_place_is_f16(Place p) { return p == PL_RB_CONV1 || p == PL_RB32 || p == PL_RB64 || p == PL_CONV_F16; }

// ---- row mixers ------------------------------------------------------------------------------------------------------
// The ops that read f32 rows (frames, L, C) from one activation slot and write rows (frames, L, cout) to another - of the
// same shape, but for the kinds that change the width -: packed weights at w_off, an optional mask, bias / batch norm / unmasked
// DyT / activation stages fused into the store.  What
// differs between them is the record below, the per-question switches of jg_model.hip (jg_mixer_*) and the kind-specific
// lines of launch_mixer (jg_run.hip).
enum MixerMask {
  MM_NONE,          // out_mask = none
  MM_KEEP,          // out_mask = in_mask (a mask slot or none)
  MM_KEEP_OR_DROP,  // out_mask = in_mask or none
  MM_OWN,           // out_mask = any mask slot or none, independent of in_mask (a mask slot or none): a mask op of the layer's
                    // own wrote it
};
struct MixerKind {
  int kind;
  const char *noun;     // in messages
  MixerMask mask;
  bool six_frames;      // mixes across the six frames of a translated window (else: along each of the id_frames rows)
  bool dilation_1;      // op.dilation must be 1
  bool in_place;        // out_buf may be in_buf
  bool same_width;      // cout = cin, and f0 is a layer norm's epsilon (else: the kind's own rule, mixer_supports)
  int prof, prof_cvt;   // JG_PROF_* class of the launch and of a layout conversion in front of it (-1: not timed)
};
static const MixerKind jg_mixer_kinds[] = {
    {JG_OP_FRAMEATTN, "frame attention", MM_NONE, true, false, true, true, JG_PROF_FRAMEATTN, JG_PROF_FRAMEATTN_CVT},
    {JG_OP_LOCALATTN, "local attention", MM_KEEP, false, true, false, true, JG_PROF_LOCALATTN, JG_PROF_LOCALATTN_CVT},
    {JG_OP_LENGTHATTN, "length attention", MM_KEEP_OR_DROP, false, false, false, true, -1, -1},
    {JG_OP_HYENA, "hyena", MM_KEEP, false, true, false, true, -1, -1},
    {JG_OP_BILSTM, "bilstm", MM_KEEP_OR_DROP, false, true, false, false, -1, -1},
    {JG_OP_MSCONV, "multi-scale conv", MM_OWN, false, true, false, false, -1, -1},
};
static inline const MixerKind *jg_mixer_kind(int kind) {      // nullptr: not a row mixer
  for (const MixerKind &k : jg_mixer_kinds)
    if (k.kind == kind) return &k;
  return nullptr;
}
static inline bool jg_op_is_mixer(int kind) { return jg_mixer_kind(kind) != nullptr; }
// FLOPs of op i (a row mixer) over nw windows of the rows r records (jg_model.hip): the model's FLOPs and the profiling bracket
double jg_mixer_flops(const jg_model *m, size_t i, const OpShape &r, int nw);

// does op read / write activation slot `buf` as a tensor (jg_prepare.hip; NMD_FINAL counts as a reader: it takes the
// slot's shape)
bool jg_op_reads(const jg_op &op, int buf);
bool jg_op_writes(const jg_op &op, int buf);

// ---- the rest ----------------------------------------------------------------------------------------------------------
int jg_prepare_tab(jg_model *m, const float *weights);          // jg_prepare.hip, in the order jg_model_create calls them
int jg_prepare_f16(jg_model *m, const float *weights);
int jg_plan_phase_split(jg_model *m, const float *weights);
int jg_plan_resblocks(jg_model *m, const float *weights);
int jg_prepare_f32(jg_model *m, const float *weights);
int jg_prepare_small(jg_model *m, const float *weights);
void jg_free_small(jg_model *m);
int64_t jg_operand_digest(const jg_model *m);                   // JG_MSTAT_OPERAND_DIGEST
const char *jg_tap_refusal(const jg_model *m, size_t i, const PlaceCtx &c, int l, char *why, size_t cap);   // jg_model.hip
int jg_tap_copy(jg_model *m, size_t i, const OpShape &r, const PlaceCtx &c, int nw, hipStream_t s);
int jg_effective_chunk(const jg_model *m, int chunk, int l, int64_t n_win);                                  // jg_run.hip
int jg_forward_chunks(jg_model *m, const std::vector<OpShape> &shp, const uint8_t *d_ids, int64_t n_win, int l, float *prediction,
                      float *reliability, float *embedding, float *nmd, int out_loc, int chunk, hipStream_t s);
int jg_forward_device_ids(jg_model *m, const uint8_t *d_ids, int64_t n_win, int l, float *prediction, float *reliability,
                          float *embedding, float *nmd, int out_loc, int chunk, hipStream_t s);

void jg_conv_inst_reset(const jg_model *m);                     // jg_run.hip: the per-op records of JG_MSTAT_TAP_INSTANCE
int64_t jg_conv_inst_get(const jg_model *m, int op, bool other);

static inline hipStream_t pick_stream(jg_engine *e, void *stream) {
  return stream != nullptr ? reinterpret_cast<hipStream_t>(stream) : e->stream;
}

template <typename T>
static int grow(T **p, int64_t *cap, int64_t need_bytes) {
  if (need_bytes <= *cap) return JG_OK;
  if (*p) JG_HIP(hipFree(*p));
  *p = nullptr;
  JG_HIP(hipMalloc(reinterpret_cast<void **>(p), (size_t)need_bytes));
  *cap = need_bytes;
  return JG_OK;
}
// ---- stream-ordered device buffers (jg_termini.hip, jg_alignpairs.hip) -------------------------------------------------
// Device allocation released with its scope - STREAM-ORDERED (hipMallocAsync / hipFreeAsync on the caller's stream): hipFree
// waits for every stream of the device, so the repeat scan - which runs beside the network's forward on a stream of its own -
// used to return only when the forward's whole queue had drained (the repeat table of a million records arrived with the
// forward's last launch, 0.2 s after the scan's own kernels had ended, and no result row could be written beside the forward).
struct DevBuf {
  void *p = nullptr;
  hipStream_t st = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFreeAsync(p, st); }
  int alloc(size_t bytes, hipStream_t s) {
    st = s;
    JG_HIP(hipMallocAsync(&p, std::max<size_t>(bytes, 1), s));
    return JG_OK;
  }
  template <typename T>
  T *as() const { return static_cast<T *>(p); }
};

template <typename T>
static int upload(DevBuf &d, const std::vector<T> &v, hipStream_t s) {
  int rc = d.alloc(v.size() * sizeof(T), s);
  if (rc != JG_OK) return rc;
  JG_HIP(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return JG_OK;
}

template <typename T>
static int download(std::vector<T> &v, const DevBuf &d, hipStream_t s) {
  JG_HIP(hipMemcpyAsync(v.data(), d.p, v.size() * sizeof(T), hipMemcpyDeviceToHost, s));
  JG_HIP(hipStreamSynchronize(s));
  return JG_OK;
}

// Stable bucketing for "one launch per kernel class, tallest class first" (workgroups are dispatched in index order, and a
// tall job costs many short ones): sorted = the n items whose cls(item) is order[0], then order[1], ..., input order inside a
// bucket; from[k] = the input index of sorted[k]; bucket b is sorted[first[b] .. first[b + 1]) (first: n_order + 1 entries,
// or nullptr).  Items of a class that `order` does not name are dropped.
template <typename T, typename ClassOf>
static void bucket_by_class(const T *items, size_t n, const int *order, int n_order, ClassOf cls, std::vector<T> &sorted,
                            std::vector<int64_t> &from, int *first = nullptr) {
  sorted.clear();
  from.clear();
  sorted.reserve(n);
  from.reserve(n);
  for (int b = 0; b < n_order; ++b) {
    if (first) first[b] = (int)sorted.size();
    for (size_t k = 0; k < n; ++k)
      if (cls(items[k]) == order[b]) { sorted.push_back(items[k]); from.push_back((int64_t)k); }
  }
  if (first) first[n_order] = (int)sorted.size();
}
#pragma GCC visibility pop
