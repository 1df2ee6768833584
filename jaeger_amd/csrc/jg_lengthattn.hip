// One TransformerEncoder along the length axis (reference: nnlib/v2/layers.py:2206-2280; the length half of
// AxialAttention, :2400-2517) as ONE launch: inside every frame row the L positions are tokens of C channels and every
// query attends every key of its row -
//   x_norm = LayerNormalization(eps 1e-6)(x)                                              :2224-2226, :2249
//   x      = x + MultiHeadAttention(H heads, key_dim D = C / H)(x_norm, x_norm)           :2227-2233, :2252-2256
//   x      = x + Dense(C)(gelu(Dense(F)(LayerNormalization(eps 1e-6)(x))))                :2237-2244, :2259-2264
// under Keras 3's implicit masks: with a mask m of the row, M[q, k] = m[q] and m[k].  A valid query takes
// its softmax over the valid keys only (a masked key's exp is exactly 0); a masked query's context is exactly zero, so
// its attention output is the projection's bias alone - and the feed-forward half runs on it as everywhere else: the
// value is real, the frame half behind this op carries it to valid positions of other frames.  Without a mask every
// position is a valid query and key.
//
// A workgroup of four waves owns a tile of T = 128 consecutive queries of one row, wave w the two 16-row blocks
// [32 w, 32 w + 32).  The dense phases are the shared code of jg_mixer_dev.h (layer norm, dense chain, feed-forward
// half) on the exact-f32 matrix cores (v_mfma_f32_16x16x4_f32: k-ordered fmaf chains from the bias).  The keys of the
// row go through LDS in chunks of 64 positions: the four waves load and normalise the chunk's rows and compute k | v
// for 16 positions each (positions at / behind L are zero-filled and invalid, never read: row r + 1 starts there); v
// rows of invalid keys are zeroed.  Scores, softmax and context are the FIRST FORM of the design: on the
// vector ALUs, one thread per (query, head) - thread t owns query t & 127 and the heads of parity t >> 7 - with an
// online softmax that advances 16 keys at a time: the 16 scores of a step live in registers, an invalid key's score is
// SELECTED to -inf (a NaN or a huge value there cannot leak), the running maximum and sum per (query, head) live in
// LDS, the context accumulates in LDS where the queries' layer-norm output lay.  All lanes of a wave share head and
// key, so k and v reads are broadcasts.  After the last chunk: context / sum (exact zero at a masked query), output
// projection onto the residual stream, LN2, the feed-forward half 16 hidden columns at a time, the op's stages, store.
//
// The op is out of place by construction: every query tile reads the whole row.
#include "jg_common.h"
#include "jg_lengthattn.h"
#include "jg_mixer_dev.h"

namespace {

constexpr int T = JG_LENGTHATTN_TILE, CH = JG_LENGTHATTN_CHUNK, STEP = JG_LENGTHATTN_STEP, QB = T / 64;
constexpr int NTHREADS = 256;
static_assert(T == 128 && CH == 64 && STEP == 16 && QB == 2, "thread mapping of lengthattn_kernel");

template <int C>
__global__ __launch_bounds__(NTHREADS) void lengthattn_kernel(JgLengthAttnArgs a) {
  extern __shared__ float ga_lds[];
  constexpr int NB = C / 16, SX = C + 2, SKV = 2 * C;
  constexpr float LOG2E = 1.44269504f;
  const int D = a.D, F = a.F, H = a.H, L = a.L, SM = 2 * H;
  float *xq = ga_lds;                    // [T][SX]  the queries' rows: LN output, then the context, the feed-forward A operand, the store
  float *qq = xq + T * SX;               // [T][SX]  q; later 16 hidden columns per wave
  float *xc = qq + T * SX;               // [CH][SX] the chunk's rows, normalised
  float *kv = xc + CH * SX;              // [CH][2 C] k | v of the chunk
  float *ml = kv + CH * SKV;             // [T][2 H] running maximum, running sum per (query, head)
  int *kvalid = reinterpret_cast<int *>(ml + T * SM);   // [CH]
  int *qvalid = kvalid + CH;                            // [T]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, j = lane >> 4;
  const int row = blockIdx.x / a.tiles, p0 = (blockIdx.x - row * a.tiles) * T;
  const JgAttnWeights w = jg_attn_weights(a.w, C, F);
  const float *__restrict__ xrow = a.x + (size_t)row * L * C;
  const uint8_t *__restrict__ mrow = a.mask != nullptr ? a.mask + (size_t)row * L : nullptr;

  // ---- the query tile: token t = position p0 + t of this row; positions at / behind L are zero rows and no queries
  jg_mixer_load_tile<C, SX, NTHREADS>(xq, T, tid, [=](int t) { return p0 + t < L; }, [=](int t) { return xrow + (size_t)(p0 + t) * C; });
  for (int t = tid; t < T; t += NTHREADS) {
    const int p = p0 + t;
    int ok = p < L;
    if (ok && mrow != nullptr) ok = mrow[p] != 0;
    qvalid[t] = ok;
  }
  __syncthreads();
  // the residual stream of the wave's 32 queries: accumulator layout (column = lane & 15 = channel, row = 4 (lane >> 4)
  // + register = position), in these registers to the store
  float *xq_w = xq + wv * (QB * 16) * SX, *qq_w = qq + wv * (QB * 16) * SX;
  f32x4 xr[QB][NB];
  jg_mixer_get<C, QB>(xr, xq_w, n, j);
  __syncthreads();
  jg_mixer_layernorm<C, NTHREADS>(xq, T, tid, a.eps);
  jg_mixer_add_bias<C, QB>(xr, w.bo, n);
  __syncthreads();
  // q of the wave's queries, all heads
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = nb * 16 + n;
    f32x4 acc[QB];
    const float bias = w.bqkv[col];
#pragma unroll
    for (int f = 0; f < QB; ++f) acc[f] = f32x4{bias, bias, bias, bias};
    jg_mixer_dense<QB, C>(xq_w, SX, w.wqkv + col, C, acc, n, j);
#pragma unroll
    for (int f = 0; f < QB; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) qq_w[(f * 16 + 4 * j + i) * SX + col] = acc[f][i];
  }
  __syncthreads();
  // the context takes the place of the queries' layer-norm output; running maximum -inf, running sum 0
  for (int q = tid; q < T * SX; q += NTHREADS) xq[q] = 0.f;
  for (int q = tid; q < T * H; q += NTHREADS) {
    ml[2 * q] = -INFINITY;
    ml[2 * q + 1] = 0.f;
  }

  // ---- the keys of the row, a chunk of CH positions at a time
  const int query = tid & (T - 1), hp = tid >> 7;
  for (int c0 = 0; c0 < L; c0 += CH) {
    jg_mixer_load_tile<C, SX, NTHREADS>(xc, CH, tid, [=](int t) { return c0 + t < L; }, [=](int t) { return xrow + (size_t)(c0 + t) * C; });
    for (int t = tid; t < CH; t += NTHREADS) {
      const int p = c0 + t;
      int ok = p < L;
      if (ok && mrow != nullptr) ok = mrow[p] != 0;
      kvalid[t] = ok;
    }
    __syncthreads();
    jg_mixer_layernorm<C, NTHREADS>(xc, CH, tid, a.eps);
    __syncthreads();
    // k | v of the wave's 16 positions; the v row of an invalid key is zero (its probability is an exact 0, and 0 * v
    // must stay 0 whatever lies there)
#pragma unroll
    for (int which = 0; which < 2; ++which)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int col = nb * 16 + n;
        f32x4 acc[1];
        const float bias = w.bqkv[(1 + which) * C + col];
        acc[0] = f32x4{bias, bias, bias, bias};
        jg_mixer_dense<1, C>(xc + wv * 16 * SX, SX, w.wqkv + (size_t)(1 + which) * C * C + col, C, acc, n, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = wv * 16 + 4 * j + i;
          kv[r * SKV + which * C + col] = (which == 1 && !kvalid[r]) ? 0.f : acc[0][i];
        }
      }
    __syncthreads();
    // scores, online softmax, context: thread = (query, heads of its parity); STEP keys at a time
    const int nk = min(CH, L - c0);
    for (int h = hp; h < H; h += 2) {
      const int hc = h * D;
      float m = ml[query * SM + 2 * h], l = ml[query * SM + 2 * h + 1];
      const float *qrow = qq + query * SX + hc;
      float *orow = xq + query * SX + hc;
      for (int t0 = 0; t0 < nk; t0 += STEP) {
        float s[STEP];
#pragma unroll
        for (int t = 0; t < STEP; ++t) s[t] = 0.f;
        for (int d = 0; d < D; ++d) {
          const float qd = qrow[d];
          const float *kc = kv + t0 * SKV + hc + d;
#pragma unroll
          for (int t = 0; t < STEP; ++t) s[t] = fmaf(qd, kc[t * SKV], s[t]);
        }
        float mx = m;
#pragma unroll
        for (int t = 0; t < STEP; ++t) {
          s[t] = kvalid[t0 + t] ? s[t] : -INFINITY;
          mx = fmaxf(mx, s[t]);
        }
        const float msafe = mx == -INFINITY ? 0.f : mx;        // (no valid key so far: every exp below is exp2(-inf) = 0)
        const float scale = __builtin_amdgcn_exp2f((m - msafe) * LOG2E);
        float lsum = 0.f;
#pragma unroll
        for (int t = 0; t < STEP; ++t) {
          s[t] = __builtin_amdgcn_exp2f((s[t] - msafe) * LOG2E);
          lsum += s[t];
        }
        l = fmaf(l, scale, lsum);
        for (int d = 0; d < D; ++d) {
          float o = orow[d] * scale;
          const float *vc = kv + t0 * SKV + C + hc + d;
#pragma unroll
          for (int t = 0; t < STEP; ++t) o = fmaf(s[t], vc[t * SKV], o);
          orow[d] = o;
        }
        m = mx;
      }
      ml[query * SM + 2 * h] = m;
      ml[query * SM + 2 * h + 1] = l;
    }
    __syncthreads();
  }

  // ---- context = accumulator / sum; a masked query's context is an exact zero
  for (int h = hp; h < H; h += 2) {
    const float l = ml[query * SM + 2 * h + 1];
    const bool ok = qvalid[query] && l > 0.f;
    const float inv = ok ? 1.0f / l : 0.f;
    float *orow = xq + query * SX + h * D;
    for (int d = 0; d < D; ++d) orow[d] = ok ? orow[d] * inv : 0.f;
  }
  __syncthreads();
  // output projection of the context onto the residual stream (x + b_o)
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const float *__restrict__ wcol = w.wo + nb * 16 + n;
#pragma unroll 4
    for (int k0 = 0; k0 < C; k0 += 4) {
      const float b = wcol[(k0 + j) * C];
#pragma unroll
      for (int f = 0; f < QB; ++f)
        xr[f][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xq_w[(f * 16 + n) * SX + k0 + j], b, xr[f][nb], 0, 0, 0);
    }
  }
  __syncthreads();

  // ---- feed-forward half: the wave's 32 rows of xq, its hidden columns in its 32 rows of q
  jg_attn_ffn<C, QB, NTHREADS>(xr, xq, T, xq_w, qq_w, w, F, a.eps, tid, n, j);

  // ---- store, with the stages the compiler fused behind the op
  jg_mixer_put<C, QB>(xq_w, xr, n, j);
  __syncthreads();
  float *__restrict__ yrow = a.y + (size_t)row * L * C;
  jg_mixer_store_tile<C, NTHREADS>(xq, T, tid, a.st, a.n_stages, [=](int t) { return p0 + t < L; }, [=](int t) { return yrow + (size_t)(p0 + t) * C; });
}

template <int C>
int launch_c(const JgLengthAttnArgs &a, int64_t lds, hipStream_t s) {
  static int64_t opened = 0;
  return jg_mixer_launch(lengthattn_kernel<C>, opened, (int64_t)a.rows * a.tiles, NTHREADS, lds, s, a);
}

}  // namespace

bool jg_lengthattn_supports(int C, int H, int F, char *why, size_t cap) { return jg_attn_supports(true, false, C, H, F, why, cap); }

int64_t jg_lengthattn_blob_floats(int C, int F) { return jg_attn_blob_floats(C, F); }

int64_t jg_lengthattn_lds_bytes(int C, int H) {
  // (the 32 x 18 hidden columns of a wave fit its 32 rows of q)
  return ((int64_t)(2 * T + CH) * (C + 2) + (int64_t)CH * 2 * C + (int64_t)T * 2 * H + CH + T) * (int64_t)sizeof(float);
}

int jg_launch_lengthattn(jg_engine *e, const JgLengthAttnArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_lengthattn_supports(a.C, a.H, a.F, why, sizeof(why)), JG_ERR_UNSUPPORTED, "length attention: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.rows >= 1 && a.L >= 1 && a.D * a.H == a.C &&
                 a.tiles == (a.L + T - 1) / T && (int64_t)a.rows * a.tiles <= 0x7fffffff,
             JG_ERR_INVALID, "length attention: bad launch arguments");
  JG_REQUIRE(a.y != a.x, JG_ERR_INVALID, "length attention: the op cannot run in place (every query tile reads the whole row)");
  const int64_t lds = jg_lengthattn_lds_bytes(a.C, a.H);
  JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "length attention: %lld bytes of LDS", (long long)lds);
  return a.C == 16 ? launch_c<16>(a, lds, s) : a.C == 32 ? launch_c<32>(a, lds, s) : launch_c<64>(a, lds, s);
}
