// MaskedBiLSTM (a forward and a backward LSTM over every frame row, their outputs side by side), jg_bilstm.hip.
#pragma once
#include "jg_common.h"

#define JG_BILSTM_ROWS 16         // rows of one workgroup: one 16-row block of the matrix cores
#define JG_BILSTM_STEPS 8         // time steps whose input projection is formed ahead of the recurrence at a time
#define JG_BILSTM_MAX_C 128
#define JG_BILSTM_IGNORE_MASK 1   // jg_op.arg bit

struct JgBilstmArgs {
  const float *x;          // (rows, L, C) f32 rows, row = window * frames + frame
  float *y;                // (rows, L, 2U), NEVER x
  const uint8_t *mask;     // (rows, L) validity, nullptr = every step is valid
  const float *w;          // packed, per direction: W [C][4U] | R [U][4U] | b [4U], column 64 w + 4 n + g = gate g of unit 16 w + n
  int rows, L, tiles;      // tiles = ceil(L / JG_BILSTM_STEPS) per row
  int C, U;
  float eps;               // unused (the row mixers' common fields)
  int n_stages;
  StageArg st[JG_MAX_STAGES];
};
// sizes the kernel covers (why: the reason when it does not)
bool jg_bilstm_supports(int C, int U, int cout, char *why, size_t cap);
int64_t jg_bilstm_blob_floats(int C, int U);
int64_t jg_bilstm_lds_bytes(int C, int U);
int jg_launch_bilstm(jg_engine *e, const JgBilstmArgs &a, hipStream_t s);
