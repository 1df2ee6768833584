// Pool-and-merge (JG_OP_POOLVEC): a masked global pool of one tensor merged into a range of a vector slot, jg_poolvec.hip.
// What a pooled branch of the reference's parallel_branches leaves (nnlib/builder.py:1109-1153), and MaskedLastPooling
// (nnlib/v2/layers.py:541-578).
#pragma once
#include "jg_common.h"

#define JG_POOLVEC_MAX_WIDTH 1024   // floats of the vector slot: the pool kernels' channel limit (one float4 a thread of 256)
#define JG_POOLVEC_MAX_FRAMES 32    // frame rows of one window the LAST kernel counts

struct JgPoolVecArgs {
  const float *x;          // (n_win, frames, L, c) f32 rows
  const uint8_t *mask;     // (n_win, frames, L) validity, nullptr = every position is valid
  float *out;              // the vector slot's rows at vec_off: (n_win, out_ld)
  int n_win, frames, L, c;
  int kind;                // JG_POOL_MAX | JG_POOL_AVG | JG_POOL_LAST
  int merge;               // JG_POOLVEC_STORE | ADD | MAX
  float scale;             // the merged value is multiplied by it
  int out_ld;
};

// why the op's fields lie outside what the kernels cover, or true
bool jg_poolvec_supports(int kind, int merge, int c, int vec_off, char *why, size_t cap);
int jg_launch_poolvec(const JgPoolVecArgs &a, hipStream_t s);
