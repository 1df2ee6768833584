// Which instantiation of the split-f16 conv template a launch runs on: a host-only restatement of the dispatch in
// jg_launch_conv_f16 (jg_conv_f16.hip) and of the per-part switch tables at the bottom of jg_conv_f16_impl.h, for the
// test readback (JG_MSTAT_TAP_INSTANCE).  Nothing here launches or decides anything; tests/test_conv_instance_reference.py
// parses the two source files and fails when this table and they disagree.
#include "jg_host.h"

namespace {
// the stage patterns of each switch table, 0 = end of list (pattern 0 itself is flagged by `plain`)
struct PatternSet {
  bool plain;
  unsigned ep[24];
};
const PatternSet ROW = {true, {
    JG_EP_NMD1,
    JG_EP_ACT1,
    JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_NORM1_DYT | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2 | JG_EP_NORM2_DYT | JG_EP_ACT2,
    JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_NMD1 | JG_EP_NORM1_DYT | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NORM2_DYT | JG_EP_ACT2,
    JG_EP_ACT1 | JG_EP_NORM2_AFF,
    JG_EP_ACT1 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ADD | JG_EP_ACT1,
    JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2,
    JG_EP_NORM1_DYT,
    JG_EP_RUNTIME,
}};
const PatternSet FLAT = {false, {
    JG_EP_ACT1,
    JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_NORM1_DYT | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2 | JG_EP_NORM2_DYT | JG_EP_ACT2,
    JG_EP_ACT1 | JG_EP_NORM2_AFF,
    JG_EP_ACT1 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NORM2_DYT | JG_EP_ACT2,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2,
    JG_EP_RUNTIME,
}};
const PatternSet LUT = {true, {
    JG_EP_NMD1,
    JG_EP_ACT1,
    JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_NORM1_DYT | JG_EP_ACT1,
    JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_NMD1 | JG_EP_NORM1_DYT | JG_EP_ACT1,
    JG_EP_ACT1 | JG_EP_NORM2_AFF,
    JG_EP_RUNTIME,
}};
const PatternSet GEOM = {true, {
    JG_EP_ACT1,
    JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ACT1,
    JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ADD | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2 | JG_EP_NORM2_AFF | JG_EP_ACT2,
    JG_EP_NORM1_DYT | JG_EP_ACT1,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1,
    JG_EP_NMD1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2,
    JG_EP_NORM1_DYT,
    JG_EP_NORM1_DYT | JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2,
    JG_EP_RUNTIME,
}};
// the patterns with a tanh-GELU build beside the general one: row and window-packed tiling of k = 5, the table variant
const unsigned HOT[] = {
    JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1,
    JG_EP_ADD | JG_EP_ACT1 | JG_EP_NMD2 | JG_EP_NORM2_AFF | JG_EP_ACT2,
};
const unsigned HOT_LUT = JG_EP_NMD1 | JG_EP_NORM1_AFF | JG_EP_ACT1;

bool has(const PatternSet &p, unsigned ep) {
  if (ep == 0u) return p.plain;
  for (unsigned q : p.ep)
    if (q == ep) return true;
  return false;
}

int64_t pack(int part, int k, unsigned ep, bool flat, int cw, bool tanh, unsigned ep_rt) {
  return JG_INST_VALID | (int64_t)part | ((int64_t)k << JG_INST_K_SHIFT) | ((int64_t)ep << JG_INST_EP_SHIFT) |
         (flat ? JG_INST_FLAT : 0) | ((int64_t)cw << JG_INST_CW_SHIFT) | (tanh ? JG_INST_TANH : 0) |
         ((int64_t)(ep == JG_EP_RUNTIME ? (ep_rt & 0x1ffu) : 0u) << JG_INST_EP_RT_SHIFT);
}
}  // namespace

// the instance jg_launch_conv_f16(a) runs on, as a JG_MSTAT_TAP_INSTANCE code; 0 when the dispatch has none (the launch
// fails there).  `a` as the launch gets it: tiling, tap range and output geometry set.
int64_t jg_conv_f16_instance(const ConvHArgs &a) {
  const bool tanh_act = a.act_kind == JG_ACT_GELU_TANH;
  if (a.lut != nullptr) {                                      // part 4: the first-layer table variant (K = 0: taps at run time)
    if (!has(LUT, a.ep)) return 0;
    if (a.cout != 128) return pack(4, 0, a.ep, false, 129, false, a.ep_rt);
    return pack(4, 0, a.ep, false, 128, a.ep == HOT_LUT && tanh_act, a.ep_rt);
  }
  if (a.k != 5 && a.k != 7 && a.k != 9) return 0;
  if (a.cw != 128) {                                           // the 64 / 32-channel tiles
    if ((a.cw != 64 && a.cw != 32) || (a.k != 5 && a.flat) || !has(GEOM, a.ep)) return 0;
    const int part = a.k == 5 ? (a.cw == 64 ? 5 : 6) : a.k == 7 ? (a.cw == 64 ? 8 : 9) : (a.cw == 64 ? 11 : 12);
    return pack(part, a.k, a.ep, a.flat != 0, a.cw, false, a.ep_rt);
  }
  if (a.cout != 128 || a.ostride != 1 || a.tap_lo != 0 || a.tap_hi != a.k - 1 || a.psplit) {   // the general 128-wide tile
    if ((a.k != 5 && a.flat) || !has(GEOM, a.ep)) return 0;
    return pack(a.k == 5 ? 7 : a.k == 7 ? 10 : 13, a.k, a.ep, a.flat != 0, 129, false, a.ep_rt);
  }
  bool hot = false;
  for (unsigned q : HOT) hot |= a.k == 5 && q == a.ep && tanh_act;
  if (a.flat) {
    if (a.k != 5 || !has(FLAT, a.ep)) return 0;
    return pack(3, 5, a.ep, true, 128, hot, a.ep_rt);
  }
  if (!has(ROW, a.ep)) return 0;
  return pack(a.k == 5 ? 1 : 2, a.k, a.ep, false, 128, hot, a.ep_rt);
}
