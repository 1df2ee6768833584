// One MultiScaleConv1D (reference: nnlib/v2/layers.py:1433-1595): n MaskedConv1Ds (:1137-1330) over the same input, every
// one with padding "same" and strides 1 and its own kernel_size k, dilation_rate d, activation, bias and mask_mode; their
// outputs side by side along the channels (merge "concat") or summed in branch order (merge "add", tf.add_n).  Per branch
//   y[t, o] = act(bias[o] + sum_{j < k} sum_{c < C} x'[t + j d - pad_left, c] w[j, c, o]),   pad_left = (k - 1) d // 2 (TF SAME)
// where x' is the input times its mask, zeros outside [0, L).  The layer's output mask is an op of its own (JG_OP_MSMASK,
// msmask_kernel below): the AND over the branches of the branch's any / majority / strict rule on the number of valid
// positions among its k taps (:1237-1254; majority = at least (k + 1) // 2 of the FULL k, at the row ends too).
//
// The final shape of the kernel:
//   * Tile.  A workgroup of 256 threads (four waves) owns JG_MSCONV_TILE = 64 consecutive positions of one row (row =
//     window * frames + frame); grid = rows x ceil(L / 64).
//   * LDS.  The 64 positions plus the halo - the largest left reach (k - 1) d // 2 and right reach (k - 1) d - (k - 1) d // 2
//     over the branches - are loaded ONCE, at the C + 2 pitch of jg_mixer_dev.h: [64 + halo_l + halo_r][C + 2] floats.  A
//     position outside [0, L) or with mask 0 is a zero row whose memory is never touched: that is both SAME padding and
//     inputs * mask, so no mask bytes are kept.  Behind it the staging tile of the output, [64][cout + 2] floats.  Worst case
//     (C 128, halo 64, cout 128) 128 x 130 x 4 + 64 x 130 x 4 = 99 840 bytes.
//   * Waves and operands.  A unit of work is one 16-column block of one branch (concat) or of the sum (add: the wave walks
//     the branches of that block in order and adds in registers); the waves take the units round robin.  A wave runs its
//     block for the four 16-token blocks of the tile at once: one read of a weight value serves four MFMAs
//     (v_mfma_f32_16x16x4_f32, exact f32).  The A operand of tap j of branch b is the same LDS tile, shifted by
//     j d_b - pad_left_b rows.
//   * Accumulation.  An accumulator starts from the branch's bias (0 without one), then one k-ordered fma chain: tap-major,
//     channel-minor.  tests/multiscale_reference.py restates this order in float32.
//   * Store.  The branch's activation first; with add the sum over the branches follows, ((y0 + y1) + y2) + y3.  The result
//     goes into the staging tile - a branch whose filters are no multiple of 16 computes a zero-padded block (the blob pads
//     its columns with zeros) and stages only its real columns, so two 8-filter branches share one 16-channel block of the
//     output - and leaves it through the stage list (bias / batch norm / unmasked DyT / activation), a lane quad writing 16
//     consecutive bytes of a position.  C and cout are run-time sizes here, so the load and the store are this file's own
//     loops in the form of jg_mixer_load_tile / jg_mixer_store_tile (which take them as template arguments).
// Every global index is row * L + position with row < rows and 0 <= position < L; the tail tile stores position < L only.
// Every output position is written, masked ones included (their value is what the valid neighbours give).
#include <string.h>

#include "jg_common.h"
#include "jg_msconv.h"
#include "jg_mixer_dev.h"

namespace {

constexpr int T = JG_MSCONV_TILE, NT = 256, NBLK = T / 16, DF = JG_MSCONV_DESC_FIELDS;
static_assert(NBLK == 4, "four 16-token blocks a wave");

__global__ __launch_bounds__(NT) void msconv_kernel(JgMsconvArgs a) {
  extern __shared__ float lds[];
  const int C = a.C, SX = C + 2, C4 = C / 4, CO = a.cout, SO = CO + 2, CO4 = CO / 4, L = a.L;
  const int span = T + a.halo_l + a.halo_r;
  float *xl = lds;                    // [span][SX]
  float *ol = xl + span * SX;         // [T][SO]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, j = lane >> 4;
  const int row = blockIdx.x / a.tiles, t0 = (blockIdx.x - row * a.tiles) * T;
  const size_t base = (size_t)row * L;
  for (int q = tid; q < span * C4; q += NT) {
    const int t = q / C4, c4 = (q - t * C4) * 4, pos = t0 - a.halo_l + t;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pos >= 0 && pos < L && (a.mask == nullptr || a.mask[base + pos] != 0))
      v = *reinterpret_cast<const float4 *>(a.x + (base + pos) * C + c4);
    float *r = xl + t * SX + c4;
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  }
  __syncthreads();
  const int *__restrict__ desc = reinterpret_cast<const int *>(a.w);
  const bool add = a.merge == JG_MSCONV_ADD;
  int n_units = 0;
  for (int b = 0; b < (add ? 1 : a.n_branches); ++b) n_units += (desc[b * DF] + 15) / 16;
  for (int u = wv; u < n_units; u += NT / 64) {
    int b_lo = 0, nb = u;
    if (!add)
      for (; b_lo < a.n_branches - 1 && nb >= (desc[b_lo * DF] + 15) / 16; ++b_lo) nb -= (desc[b_lo * DF] + 15) / 16;
    const int b_hi = add ? a.n_branches : b_lo + 1;
    const int col = nb * 16 + n;
    f32x4 tot[NBLK] = {};
    for (int b = b_lo; b < b_hi; ++b) {
      const int filters = desc[b * DF], taps = desc[b * DF + 1], dil = desc[b * DF + 2], act = desc[b * DF + 3];
      const int fpad = (filters + 15) & ~15, pad_left = ((taps - 1) * dil) / 2;
      const float *__restrict__ wk = a.w + desc[b * DF + 7] + col;              // [taps][C][fpad], this lane's column
      const float bias = wk[(size_t)taps * C * fpad];
      f32x4 acc[NBLK];
#pragma unroll
      for (int f = 0; f < NBLK; ++f) acc[f] = f32x4{bias, bias, bias, bias};
      for (int tap = 0; tap < taps; ++tap) {
        const float *ar = xl + (a.halo_l + tap * dil - pad_left + n) * SX + j;
        const float *__restrict__ wt = wk + (size_t)tap * C * fpad + (size_t)j * fpad;
#pragma unroll 4
        for (int k0 = 0; k0 < C; k0 += 4) {
          const float bv = wt[(size_t)k0 * fpad];
#pragma unroll
          for (int f = 0; f < NBLK; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[f * 16 * SX + k0], bv, acc[f], 0, 0, 0);
        }
      }
#pragma unroll
      for (int f = 0; f < NBLK; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = jg_apply_act(acc[f][i], act);
          tot[f][i] = b == b_lo ? v : tot[f][i] + v;
        }
    }
    if (col < desc[b_lo * DF]) {
      float *o = ol + (add ? 0 : desc[b_lo * DF + 6]) + col;
#pragma unroll
      for (int f = 0; f < NBLK; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[(f * 16 + 4 * j + i) * SO] = tot[f][i];
    }
  }
  __syncthreads();
  for (int q = tid; q < T * CO4; q += NT) {
    const int t = q / CO4, c4 = (q - t * CO4) * 4, pos = t0 + t;
    if (pos >= L) continue;
    const float *r = ol + t * SO + c4;
    float4 v;
    v.x = jg_mixer_stages(r[0], a.st, a.n_stages, c4);
    v.y = jg_mixer_stages(r[1], a.st, a.n_stages, c4 + 1);
    v.z = jg_mixer_stages(r[2], a.st, a.n_stages, c4 + 2);
    v.w = jg_mixer_stages(r[3], a.st, a.n_stages, c4 + 3);
    *reinterpret_cast<float4 *>(a.y + (base + pos) * CO + c4) = v;
  }
}

// one thread a position
__global__ __launch_bounds__(256) void msmask_kernel(const uint8_t *__restrict__ in, int64_t n_pos, int L, const int *__restrict__ desc,
                                                     int n_branches, uint8_t *__restrict__ out) {
  const int64_t idx = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (idx >= n_pos) return;
  const int64_t row = idx / L;
  const int t = (int)(idx - row * L);
  const uint8_t *r = in + row * L;
  bool ok = true;
  for (int b = 0; b < n_branches; ++b) {
    const int taps = desc[b * DF + 1], dil = desc[b * DF + 2], mode = desc[b * DF + 4];
    const int pad_left = ((taps - 1) * dil) / 2;
    int cnt = 0;
    for (int tap = 0; tap < taps; ++tap) {
      const int p = t - pad_left + tap * dil;
      cnt += (p >= 0 && p < L && r[p] != 0) ? 1 : 0;
    }
    ok = ok && (mode == JG_MASK_ANY ? cnt > 0 : mode == JG_MASK_MAJORITY ? cnt >= (taps + 1) / 2 : cnt == taps);
  }
  out[idx] = ok ? 1 : 0;
}

}  // namespace

bool jg_msconv_supports(int C, int n_branches, int cout, int merge, char *why, size_t cap) {
  if (C < 16 || C > JG_MSCONV_MAX_C || C % 16 != 0) {
    snprintf(why, cap, "%d incoming channels (a multiple of 16 up to %d)", C, JG_MSCONV_MAX_C);
    return false;
  }
  if (n_branches < 1 || n_branches > JG_MSCONV_MAX_BRANCHES) {
    snprintf(why, cap, "%d branches (1 to %d)", n_branches, JG_MSCONV_MAX_BRANCHES);
    return false;
  }
  if (cout < 16 || cout > JG_MSCONV_MAX_C || cout % 16 != 0) {
    snprintf(why, cap, "%d output channels (a multiple of 16 up to %d)", cout, JG_MSCONV_MAX_C);
    return false;
  }
  if (merge != JG_MSCONV_CONCAT && merge != JG_MSCONV_ADD) {
    snprintf(why, cap, "merge kind %d (0 concat, 1 add)", merge);
    return false;
  }
  return true;
}

int jg_msconv_read_desc(const float *blob, int64_t avail, int C, int n_branches, int cout, int merge, JgMsconvDesc *d, char *why, size_t cap) {
  if (!jg_msconv_supports(C, n_branches, cout, merge, why, cap)) return JG_ERR_UNSUPPORTED;
  if (avail < JG_MSCONV_DESC_FLOATS) {
    snprintf(why, cap, "a descriptor outside the weight blob");
    return JG_ERR_INVALID;
  }
  memset(d, 0, sizeof(*d));
  d->n = n_branches;
  d->floats = JG_MSCONV_DESC_FLOATS;
  int next_ch = 0;
  for (int b = 0; b < n_branches; ++b) {
    JgMsconvBranch &br = d->b[b];
    memcpy(&br, blob + b * JG_MSCONV_DESC_FIELDS, sizeof(br));
    if (br.filters < 8 || br.filters > JG_MSCONV_MAX_C || br.filters % 8 != 0) {
      snprintf(why, cap, "branch %d: %d filters (a multiple of 8 up to %d)", b, br.filters, JG_MSCONV_MAX_C);
      return JG_ERR_UNSUPPORTED;
    }
    if (br.taps < 1 || br.taps > JG_MSCONV_MAX_TAPS) {
      snprintf(why, cap, "branch %d: kernel_size %d (1 to %d)", b, br.taps, JG_MSCONV_MAX_TAPS);
      return JG_ERR_UNSUPPORTED;
    }
    if (br.dilation < 1 || (int64_t)(br.taps - 1) * br.dilation > JG_MSCONV_MAX_SPAN) {
      snprintf(why, cap, "branch %d: (kernel_size - 1) x dilation_rate = %lld (dilation_rate at least 1, the product up to %d)", b,
               (long long)(br.taps - 1) * br.dilation, JG_MSCONV_MAX_SPAN);
      return JG_ERR_UNSUPPORTED;
    }
    if (br.act < JG_ACT_NONE || br.act > JG_ACT_SIGMOID || br.mask_mode < JG_MASK_ANY || br.mask_mode > JG_MASK_STRICT ||
        (br.has_bias != 0 && br.has_bias != 1)) {
      snprintf(why, cap, "branch %d: activation %d, mask mode %d, has-bias %d", b, br.act, br.mask_mode, br.has_bias);
      return JG_ERR_INVALID;
    }
    const int fpad = (br.filters + 15) & ~15;
    const int64_t need = (int64_t)br.taps * C * fpad + fpad;
    if (br.w_off < JG_MSCONV_DESC_FLOATS || (int64_t)br.w_off + need > avail) {
      snprintf(why, cap, "branch %d: weights at %d (+ %lld floats) outside the blob", b, br.w_off, (long long)need);
      return JG_ERR_INVALID;
    }
    if (merge == JG_MSCONV_CONCAT ? br.ch_off != next_ch : (br.ch_off != 0 || br.filters != cout)) {
      snprintf(why, cap, merge == JG_MSCONV_CONCAT ? "branch %d: channel offset %d, %d filters (the branches tile [0, %d) in order)"
                                                   : "branch %d: channel offset %d, %d filters (summed branches have the output's %d)",
               b, br.ch_off, br.filters, cout);
      return JG_ERR_INVALID;
    }
    next_ch += br.filters;
    const int reach = (br.taps - 1) * br.dilation;
    d->halo_l = reach / 2 > d->halo_l ? reach / 2 : d->halo_l;
    d->halo_r = reach - reach / 2 > d->halo_r ? reach - reach / 2 : d->halo_r;
    d->floats = (int64_t)br.w_off + need > d->floats ? (int64_t)br.w_off + need : d->floats;
    d->macs += (int64_t)br.taps * br.filters;
  }
  if (merge == JG_MSCONV_CONCAT && next_ch != cout) {
    snprintf(why, cap, "branches of %d filters in all for %d output channels", next_ch, cout);
    return JG_ERR_INVALID;
  }
  return JG_OK;
}

int64_t jg_msconv_lds_bytes(int C, int cout, int halo_l, int halo_r) {
  return ((int64_t)(T + halo_l + halo_r) * (C + 2) + (int64_t)T * (cout + 2)) * (int64_t)sizeof(float);
}

int jg_launch_msconv(jg_engine *e, const JgMsconvArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_msconv_supports(a.C, a.n_branches, a.cout, a.merge, why, sizeof(why)), JG_ERR_UNSUPPORTED, "msconv: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.rows >= 1 && a.L >= 1 && a.tiles == (a.L + T - 1) / T &&
                 a.halo_l >= 0 && a.halo_r >= 0 && a.halo_l + a.halo_r <= JG_MSCONV_MAX_SPAN && (int64_t)a.rows * a.tiles <= 0x7fffffff,
             JG_ERR_INVALID, "msconv: bad launch arguments");
  JG_REQUIRE(a.y != a.x, JG_ERR_INVALID, "msconv: the op cannot run in place");
  const int64_t lds = jg_msconv_lds_bytes(a.C, a.cout, a.halo_l, a.halo_r);
  JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "msconv: %lld bytes of LDS", (long long)lds);
  static int64_t opened = 0;
  return jg_mixer_launch(msconv_kernel, opened, (int64_t)a.rows * a.tiles, NT, lds, s, a);
}

int jg_launch_msmask(const uint8_t *in, int rows, int L, const float *desc, int n_branches, uint8_t *out, hipStream_t s) {
  if (rows == 0 || L <= 0) return JG_OK;
  JG_REQUIRE(in != nullptr && out != nullptr && in != out && desc != nullptr && n_branches >= 1 && n_branches <= JG_MSCONV_MAX_BRANCHES,
             JG_ERR_INVALID, "msmask: bad launch arguments");
  const int64_t n_pos = (int64_t)rows * L;
  hipLaunchKernelGGL(msmask_kernel, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, s, in, n_pos, L,
                     reinterpret_cast<const int *>(desc), n_branches, out);
  JG_HIP(hipGetLastError());
  return JG_OK;
}
