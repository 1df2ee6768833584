// One HyenaBlock (reference: nnlib/v2/layers.py:2724-3153) over the frame rows of a window.  With a mask m of the row -
//   x' = x * m;  n = LayerNormalization(eps 1e-6)(x') * m                                  :3109-3122
//   p_k = n @ W_k, k = 0 .. order (no bias);  z = p_0                                      :2989-2992
//   z = p_{i + 1} * causal_conv(z, h_i), i = 0 .. order - 1                                :2996-3000
//       causal_conv(z, h)[t, c] = sum over s <= t of h[t - s, c] z[s, c]                   :2724-2763
//   y = z (@ W_o + b_o with output_projection);  out = (y + x') * m                        :3125-3133
// and without one every `* m` is absent.  The filters h_i depend on weights and position only: the host tables them
// once (program.py: hyena_filter_tables) and the op's blob carries the table, lag-indexed, [order][table_rows][C]; with
// filter_normalize a second table holds the running sum of squares over the lag, so that the L2 norm over the l
// positions of a call is one lookup and divide_no_nan a zero test.
//
// FIRST FORM: three kernels, 2 + order launches, p_0 .. p_order through a scratch region in global
// memory that the shape walk sizes - any row length up to the table's rows runs, and no phase holds more than a tile
// in LDS.  Every workgroup owns a tile of 64 positions of one row and all C channels:
//   * hyena_proj_kernel   loads the tile (masked positions as zeros), normalises (gamma / beta are folded into the
//     projections on the host), and forms p_0 .. p_order on the exact-f32 matrix cores (v_mfma_f32_16x16x4_f32: a
//     k-ordered fmaf chain from the folded bias), one 16-position block per wave; masked positions store exact zeros.
//   * hyena_conv_kernel   one convolution and its gate, on the vector ALUs: a thread owns one channel and C / 4
//     consecutive positions of the tile.  The z prefix and the filter slice go through LDS in chunks of 64 earlier
//     positions (127 lags); inside a chunk a thread walks the sources in ascending order with an fmaf chain from zero,
//     and adds the chunk's partial sum to its running sum - partial sums per chunk, not one chain over the row (DESIGN
//     3.8).  Lags below zero are zero rows of the LDS slice: the diagonal chunk needs no branch inside a block of
//     sources, and the blocks that lie wholly behind a thread's positions are skipped.  The gate p_{i + 1} is read and
//     z_{i + 1} written at the same address by the same thread; other workgroups read z_i only.
//   * hyena_out_kernel    the output projection (matrix cores) if there is one, the residual, the mask, the op's
//     stages, the store.
// Rows never touch each other: every index is row * L + position with position < L, positions at / behind L are
// zero-filled in LDS and never stored.
#include "jg_common.h"
#include "jg_hyena.h"
#include "jg_mixer_dev.h"

namespace {

constexpr int T = JG_HYENA_TILE, CH = JG_HYENA_CHUNK, NTHREADS = 256;
static_assert(T == 64 && CH == 64, "thread mapping of the hyena kernels");

// ---- phase 1: p_0 .. p_order of a tile ------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(NTHREADS) void hyena_proj_kernel(JgHyenaArgs a) {
  constexpr int NB = C / 16, SX = C + 2;
  __shared__ float xn[T * SX];
  __shared__ int valid[T];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, j = lane >> 4;
  const int L = a.L, row = blockIdx.x / a.tiles, p0 = (blockIdx.x - row * a.tiles) * T;
  const float *__restrict__ xrow = a.x + (size_t)row * L * C;
  const uint8_t *__restrict__ mrow = a.mask != nullptr ? a.mask + (size_t)row * L : nullptr;
  jg_mixer_load_tile<C, SX, NTHREADS>(xn, T, tid, [=](int t) { return p0 + t < L && (mrow == nullptr || mrow[p0 + t] != 0); },
                                      [=](int t) { return xrow + (size_t)(p0 + t) * C; });
  for (int t = tid; t < T; t += NTHREADS) {
    const int p = p0 + t;
    valid[t] = p < L && (mrow == nullptr || mrow[p] != 0);
  }
  __syncthreads();
  jg_mixer_layernorm<C, NTHREADS>(xn, T, tid, a.eps);
  __syncthreads();
  const float *__restrict__ wp = a.w;                                   // [order + 1][C][C] (input channel, output channel)
  const float *__restrict__ bp = wp + (size_t)(a.order + 1) * C * C;    // [order + 1][C]
  const size_t plane = (size_t)a.rows * L * C;
  for (int k = 0; k <= a.order; ++k) {
    float *__restrict__ prow = a.scratch + k * plane + (size_t)row * L * C;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int col = nb * 16 + n;
      const float bias = bp[k * C + col];
      f32x4 acc[1] = {f32x4{bias, bias, bias, bias}};
      jg_mixer_dense<1, C>(xn + wv * 16 * SX, SX, wp + (size_t)k * C * C + col, C, acc, n, j);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = wv * 16 + 4 * j + i, p = p0 + r;
        if (p < L) prow[(size_t)p * C + col] = valid[r] ? acc[0][i] : 0.f;
      }
    }
  }
}

// ---- phase 2: z_out = gate * causal_conv(z_in, h), one launch per order ---------------------------------------------
template <int C>
__global__ __launch_bounds__(NTHREADS) void hyena_conv_kernel(const float *__restrict__ zin, float *gate_out, const float *__restrict__ h,
                                                              const float *__restrict__ ssq, int L, int tiles, int table_rows) {
  constexpr int NP = C / 4, NG = NTHREADS / C, HR = T + CH - 1;
  static_assert(NG * NP == T && CH % NP == 0, "a thread owns C / 4 consecutive positions of one channel");
  __shared__ float zl[CH * C];
  __shared__ float hl[(HR + 1) * C];
  const int tid = threadIdx.x, c = tid % C, g = tid / C;
  const int row = blockIdx.x / tiles, t0 = (blockIdx.x - row * tiles) * T;
  const float *__restrict__ zrow = zin + (size_t)row * L * C;
  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.f;
  for (int s0 = 0; s0 <= t0; s0 += CH) {
    __syncthreads();
    jg_mixer_load_tile<C, C, NTHREADS>(zl, CH, tid, [=](int t) { return s0 + t < L; }, [=](int t) { return zrow + (size_t)(s0 + t) * C; });
    // slice row jr holds lag t0 - s0 - (CH - 1) + jr; lags below zero (the diagonal chunk) and at / behind the table: zeros
    const int lag0 = t0 - s0 - (CH - 1);
    jg_mixer_load_tile<C, C, NTHREADS>(hl, HR, tid, [=](int jr) { return lag0 + jr >= 0 && lag0 + jr < table_rows; },
                                       [=](int jr) { return h + (size_t)(lag0 + jr) * C; });
    __syncthreads();
    float part[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) part[p] = 0.f;
    // output g NP + p, source sb + u: slice row (g NP + p) - (sb + u) + CH - 1 = base + (p - u), in [0, HR)
    // (the diagonal chunk: sources behind the thread's last position meet negative lags alone - zero rows - and are skipped)
    const int sb_end = s0 == t0 ? (g + 1) * NP : CH;
    for (int sb = 0; sb < sb_end; sb += NP) {
      const int base = g * NP - sb + (CH - 1);
      float zz[NP], hh[2 * NP - 1];
#pragma unroll
      for (int u = 0; u < NP; ++u) zz[u] = zl[(sb + u) * C + c];
#pragma unroll
      for (int d = 0; d < 2 * NP - 1; ++d) hh[d] = hl[(base + d - (NP - 1)) * C + c];
#pragma unroll
      for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int p = 0; p < NP; ++p) part[p] = fmaf(hh[p - u + NP - 1], zz[u], part[p]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] += part[p];
  }
  // filter_normalize: h / ||h[0 .. L)|| per channel, divide_no_nan - applied to the sum (the convolution is linear)
  float inv = 1.f;
  if (ssq != nullptr) {
    const float s2 = ssq[(size_t)(L - 1) * C + c];
    inv = s2 > 0.f ? 1.0f / sqrtf(s2) : 0.f;
  }
  float *grow = gate_out + (size_t)row * L * C;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int t = t0 + g * NP + p;
    if (t < L) {
      const size_t at = (size_t)t * C + c;
      grow[at] = grow[at] * (acc[p] * inv);
    }
  }
}

// ---- phase 3: output projection, residual, mask, stages, store -------------------------------------------------------
template <int C>
__global__ __launch_bounds__(NTHREADS) void hyena_out_kernel(JgHyenaArgs a, const float *__restrict__ z) {
  constexpr int NB = C / 16, SX = C + 2;
  __shared__ float yl[T * SX];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, j = lane >> 4;
  const int L = a.L, row = blockIdx.x / a.tiles, p0 = (blockIdx.x - row * a.tiles) * T;
  const float *__restrict__ zrow = z + (size_t)row * L * C;
  jg_mixer_load_tile<C, SX, NTHREADS>(yl, T, tid, [=](int t) { return p0 + t < L; }, [=](int t) { return zrow + (size_t)(p0 + t) * C; });
  __syncthreads();
  if (a.out_proj) {
    const float *__restrict__ wo = a.w + (size_t)(a.order + 1) * C * C + (size_t)(a.order + 1) * C;   // [C][C]
    const float *__restrict__ bo = wo + (size_t)C * C;                                                // [C]
    f32x4 y[1][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float bias = bo[nb * 16 + n];
      f32x4 acc[1] = {f32x4{bias, bias, bias, bias}};
      jg_mixer_dense<1, C>(yl + wv * 16 * SX, SX, wo + nb * 16 + n, C, acc, n, j);
      y[0][nb] = acc[0];
    }
    __syncthreads();
    jg_mixer_put<C, 1>(yl + wv * 16 * SX, y, n, j);
    __syncthreads();
  }
  const float *__restrict__ xrow = a.x + (size_t)row * L * C;
  const uint8_t *__restrict__ mrow = a.mask != nullptr ? a.mask + (size_t)row * L : nullptr;
  float *__restrict__ yrow = a.y + (size_t)row * L * C;
  for (int q = tid; q < T * (C / 4); q += NTHREADS) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4, p = p0 + t;
    if (p >= L) continue;
    const float *r = yl + t * SX + c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);           // a masked position: (y + x m) m = 0
    if (mrow == nullptr || mrow[p] != 0) {
      const float4 xv = *reinterpret_cast<const float4 *>(xrow + (size_t)p * C + c4);
      v = make_float4(r[0] + xv.x, r[1] + xv.y, r[2] + xv.z, r[3] + xv.w);
    }
    v.x = jg_mixer_stages(v.x, a.st, a.n_stages, c4);
    v.y = jg_mixer_stages(v.y, a.st, a.n_stages, c4 + 1);
    v.z = jg_mixer_stages(v.z, a.st, a.n_stages, c4 + 2);
    v.w = jg_mixer_stages(v.w, a.st, a.n_stages, c4 + 3);
    *reinterpret_cast<float4 *>(yrow + (size_t)p * C + c4) = v;
  }
}

template <int C>
int launch_c(const JgHyenaArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.rows * a.tiles)), block(NTHREADS);
  const size_t plane = (size_t)a.rows * a.L * C;
  hipLaunchKernelGGL(hyena_proj_kernel<C>, grid, block, 0, s, a);
  JG_HIP(hipGetLastError());
  const int64_t flags = (a.out_proj ? JG_HYENA_OUT_PROJ : 0) | (a.normalize ? JG_HYENA_NORMALIZE : 0);
  const float *h = a.w + jg_hyena_blob_floats(C, a.order, 0, flags & JG_HYENA_OUT_PROJ);   // (0 table rows: the weights in front of the tables)
  const float *ssq = a.normalize ? h + (size_t)a.order * a.table_rows * C : nullptr;
  for (int i = 0; i < a.order; ++i) {
    hipLaunchKernelGGL(hyena_conv_kernel<C>, grid, block, 0, s, a.scratch + i * plane, a.scratch + (i + 1) * plane,
                       h + (size_t)i * a.table_rows * C, ssq != nullptr ? ssq + (size_t)i * a.table_rows * C : nullptr, a.L, a.tiles,
                       a.table_rows);
    JG_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(hyena_out_kernel<C>, grid, block, 0, s, a, a.scratch + a.order * plane);
  JG_HIP(hipGetLastError());
  return JG_OK;
}

}  // namespace

bool jg_hyena_supports(int C, int order, int table_rows, char *why, size_t cap) {
  if (C != 16 && C != 32 && C != 64) {
    snprintf(why, cap, "%d channels (the kernels cover 16, 32 and 64)", C);
    return false;
  }
  if (order < 1 || order > JG_HYENA_MAX_ORDER) {
    snprintf(why, cap, "order %d (1 to %d)", order, JG_HYENA_MAX_ORDER);
    return false;
  }
  if (table_rows < 1) {
    snprintf(why, cap, "a filter table of %d rows", table_rows);
    return false;
  }
  return true;
}

int64_t jg_hyena_blob_floats(int C, int order, int table_rows, int flags) {
  int64_t n = (int64_t)(order + 1) * C * C + (int64_t)(order + 1) * C;
  if (flags & JG_HYENA_OUT_PROJ) n += (int64_t)C * C + C;
  n += (int64_t)order * table_rows * C * ((flags & JG_HYENA_NORMALIZE) ? 2 : 1);
  return n;
}

int64_t jg_hyena_row_scratch(int C, int order, int L) { return (int64_t)(order + 1) * L * C; }

int jg_launch_hyena(jg_engine *e, const JgHyenaArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_hyena_supports(a.C, a.order, a.table_rows, why, sizeof(why)), JG_ERR_UNSUPPORTED, "hyena: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.scratch != nullptr && a.rows >= 1 && a.L >= 1 &&
                 a.tiles == (a.L + T - 1) / T && (int64_t)a.rows * a.tiles <= 0x7fffffff,
             JG_ERR_INVALID, "hyena: bad launch arguments");
  JG_REQUIRE(a.y != a.x, JG_ERR_INVALID, "hyena: the op cannot run in place");
  JG_REQUIRE(a.L <= a.table_rows, JG_ERR_UNSUPPORTED, "hyena: rows of %d positions, the filter table holds %d", a.L, a.table_rows);
  return a.C == 16 ? launch_c<16>(a, s) : a.C == 32 ? launch_c<32>(a, s) : launch_c<64>(a, s);
}
