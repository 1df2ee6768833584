// HyenaBlock (layer norm -> HyenaOperator: projections, `order` gated causal long convolutions -> optional output
// projection -> residual), jg_hyena.hip.
#pragma once
#include "jg_common.h"

#define JG_HYENA_TILE 64         // positions of one workgroup, in all three phases
#define JG_HYENA_CHUNK 64        // earlier positions (and the filter lags that go with them) through LDS at a time; one partial sum per chunk
#define JG_HYENA_MAX_ORDER 4
#define JG_HYENA_OUT_PROJ 1      // jg_op.arg bits
#define JG_HYENA_NORMALIZE 2

struct JgHyenaArgs {
  const float *x;          // (rows, L, C) f32 rows, row = window * frames + frame
  float *y;                // same geometry, NEVER x (the last phase reads x while other workgroups store)
  const uint8_t *mask;     // (rows, L) validity, nullptr = no mask (no multiply anywhere)
  const float *w;          // packed: wp [order + 1][C][C] | bp [order + 1][C] | (out_proj: wo [C][C] | bo [C]) | h [order][table_rows][C] | (normalize: ssq [order][table_rows][C])
  float *scratch;          // [order + 1][rows][L][C]: p_0 .. p_order; z_{i + 1} takes p_{i + 1}'s place
  int rows, L, tiles;      // tiles = ceil(L / JG_HYENA_TILE) per row
  int C, order, table_rows;
  int out_proj, normalize;
  float eps;               // of the layer norm
  int n_stages;
  StageArg st[JG_MAX_STAGES];
};
// sizes the kernels cover (why: the reason when they do not)
bool jg_hyena_supports(int C, int order, int table_rows, char *why, size_t cap);
int64_t jg_hyena_blob_floats(int C, int order, int table_rows, int flags);
// floats of scratch one row of L positions needs
int64_t jg_hyena_row_scratch(int C, int order, int L);
int jg_launch_hyena(jg_engine *e, const JgHyenaArgs &a, hipStream_t s);
