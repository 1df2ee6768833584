// MultiScaleConv1D (parallel MaskedConv1Ds over one input, concatenated or summed) and its output-mask rule, jg_msconv.hip.
#pragma once
#include "jg_common.h"

#define JG_MSCONV_TILE 64           // consecutive positions of one row a workgroup owns
#define JG_MSCONV_MAX_BRANCHES 4
#define JG_MSCONV_MAX_C 128         // incoming channels, a branch's filters, the output width
#define JG_MSCONV_MAX_TAPS 15
#define JG_MSCONV_MAX_SPAN 64       // (kernel_size - 1) * dilation_rate of a branch
#define JG_MSCONV_CONCAT 0          // jg_op.arg: the merge kind
#define JG_MSCONV_ADD 1
#define JG_MSCONV_DESC_FIELDS 8     // int32 bit patterns per branch at the head of the blob, in the order of JgMsconvBranch
#define JG_MSCONV_DESC_FLOATS (JG_MSCONV_MAX_BRANCHES * JG_MSCONV_DESC_FIELDS)

// one branch as the descriptor at the head of the packed blob holds it (program.py: pack_msconv).  Behind the descriptor,
// at w_off floats from the blob's start: the kernel [taps][cin][fpad] (fpad = filters rounded up to 16, the padding columns
// zeros) and the bias [fpad] (zeros without one)
struct JgMsconvBranch {
  int filters, taps, dilation, act, mask_mode, has_bias, ch_off, w_off;
};
struct JgMsconvDesc {
  int n;
  JgMsconvBranch b[JG_MSCONV_MAX_BRANCHES];
  int halo_l, halo_r;      // the largest left / right reach over the branches: (k-1)d // 2 and (k-1)d - (k-1)d // 2
  int64_t floats;          // of the whole blob
  int64_t macs;            // sum over the branches of taps x filters (x cin = multiply-adds per position)
};

struct JgMsconvArgs {
  const float *x;          // (rows, L, C) f32 rows, row = window * frames + frame
  float *y;                // (rows, L, cout), NEVER x
  const uint8_t *mask;     // (rows, L) validity of the input, nullptr = every position is valid
  const float *w;          // the packed blob: descriptor, then per branch kernel | bias
  int rows, L, tiles;      // tiles = ceil(L / JG_MSCONV_TILE) per row
  int C, cout, n_branches, merge;
  int halo_l, halo_r;
  float eps;               // unused (the row mixers' common fields)
  int n_stages;
  StageArg st[JG_MAX_STAGES];
};

// sizes the kernel covers, from the op's fields alone (why: the reason when it does not)
bool jg_msconv_supports(int C, int n_branches, int cout, int merge, char *why, size_t cap);
// the descriptor of an op with these fields out of the `avail` floats at its w_off: every field inside the kernel's sizes,
// every offset inside the blob, the channel offsets tiling [0, cout) for concat.  JG_OK, or JG_ERR_UNSUPPORTED (a size outside
// the kernel's) / JG_ERR_INVALID (a malformed descriptor) with the reason in why
int jg_msconv_read_desc(const float *blob, int64_t avail, int C, int n_branches, int cout, int merge, JgMsconvDesc *d, char *why, size_t cap);
int64_t jg_msconv_lds_bytes(int C, int cout, int halo_l, int halo_r);
int jg_launch_msconv(jg_engine *e, const JgMsconvArgs &a, hipStream_t s);
// out[row][t] = AND over the branches of the branch's any / majority / strict rule on the valid positions among its taps
int jg_launch_msmask(const uint8_t *in, int rows, int L, const float *desc, int n_branches, uint8_t *out, hipStream_t s);
