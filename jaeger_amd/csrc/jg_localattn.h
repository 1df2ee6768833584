// LocalAttention, one block of it, as one launch (jg_localattn.hip).
#pragma once
#include "jg_common.h"

#define JG_LOCALATTN_TILE 80          // query positions of one work item (five 16-row blocks of the matrix cores)
#define JG_LOCALATTN_MAX_HALF 32      // largest half-window (two halo blocks on each side of the tile)

struct JgLocalAttnArgs {
  const float *x;          // (rows, L, C) f32 rows, row = window * 6 + frame
  float *y;                // same geometry, NEVER x: a neighbouring tile reads this tile's positions as its halo
  const uint8_t *mask;     // (rows, L) key validity, nullptr = every position of [0, L) is a key
  const float *w;          // packed weights: JgAttnWeights (jg_mixer_dev.h)
  int rows, L, tiles;      // tiles = ceil(L / JG_LOCALATTN_TILE) per row
  int C, H, D, F;          // channels, heads, key_dim = C / H, feed-forward width
  int half;                // query q attends keys k with |q - k| <= half
  float eps;               // of both layer norms
  int n_stages;
  StageArg st[JG_MAX_STAGES];
};
// sizes the kernel covers (why: the reason when it does not)
bool jg_localattn_supports(int C, int H, int F, int half, char *why, size_t cap);
int64_t jg_localattn_blob_floats(int C, int F);
int64_t jg_localattn_lds_bytes(int C, int D, int half);
int jg_launch_localattn(jg_engine *e, const JgLocalAttnArgs &a, hipStream_t s);
