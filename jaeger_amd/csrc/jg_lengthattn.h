// TransformerEncoder along the length axis (the length half of AxialAttention), as one launch (jg_lengthattn.hip).
#pragma once
#include "jg_common.h"

#define JG_LENGTHATTN_TILE 128        // query positions of one workgroup (four waves, two 16-row blocks each)
#define JG_LENGTHATTN_CHUNK 64        // key positions that go through LDS at a time (one 16-row block per wave)
#define JG_LENGTHATTN_STEP 16         // keys per update of the online softmax (scores of one step live in registers)

struct JgLengthAttnArgs {
  const float *x;          // (rows, L, C) f32 rows, row = window * frames + frame
  float *y;                // same geometry, NEVER x: every query tile reads the whole row
  const uint8_t *mask;     // (rows, L) query / key validity, nullptr = every position of [0, L) is valid
  const float *w;          // packed weights: JgAttnWeights (jg_mixer_dev.h)
  int rows, L, tiles;      // tiles = ceil(L / JG_LENGTHATTN_TILE) per row
  int C, H, D, F;          // channels, heads, key_dim = C / H, feed-forward width
  float eps;               // of both layer norms
  int n_stages;
  StageArg st[JG_MAX_STAGES];
};
// sizes the kernel covers (why: the reason when it does not)
bool jg_lengthattn_supports(int C, int H, int F, char *why, size_t cap);
int64_t jg_lengthattn_blob_floats(int C, int F);
int64_t jg_lengthattn_lds_bytes(int C, int H);
int jg_launch_lengthattn(jg_engine *e, const JgLengthAttnArgs &a, hipStream_t s);
