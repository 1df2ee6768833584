// CrossFrameAttention as one launch (jg_frameattn.hip).
#pragma once
#include "jg_common.h"

struct JgFrameAttnArgs {
  const float *x;          // (n_win * 6, L, C) f32 rows, row = window * 6 + frame
  float *y;                // same geometry (may be x: a tile is read whole before it is written)
  const float *w;          // packed weights: JgAttnWeights (jg_mixer_dev.h)
  int n_win, L, tiles;     // tiles = ceil(L / 16) position tiles per window
  int C, H, D, F;          // channels, heads, key_dim = C / H, feed-forward width (0 = no feed-forward half)
  float eps;               // of both layer norms
  int n_stages;
  StageArg st[JG_MAX_STAGES];
};
// sizes the kernel covers (why: the reason when it does not)
bool jg_frameattn_supports(int C, int H, int F, char *why, size_t cap);
int64_t jg_frameattn_blob_floats(int C, int F);
int jg_launch_frameattn(jg_engine *e, const JgFrameAttnArgs &a, hipStream_t s);
