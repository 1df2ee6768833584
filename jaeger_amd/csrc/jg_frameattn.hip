// CrossFrameAttention (reference: nnlib/v2/layers.py:2283-2384) as ONE launch: at every position of a window the six
// reading frames are six tokens of C channels -
//   x_norm = LayerNormalization(eps 1e-6)(x)                      :2321-2323, :2362
//   x      = x + MultiHeadAttention(H heads, key_dim D = C / H)(x_norm, x_norm) over the six tokens   :2324-2330, :2363-2367
//   x      = x + Dense(C)(gelu(Dense(F)(LayerNormalization(eps 1e-6)(x))))          (use_ffn)          :2335-2347, :2370-2376
// Nothing couples neighbouring positions, so a wave owns a tile of 16 positions x 6 frames = 96 tokens = six 16-row blocks
// of the matrix cores (block f = frame f, row = position) and carries it from the load to the store: the tensor is read
// once and written once; LN outputs, q / k / v, scores, probabilities, context, the projection and the hidden layer of the
// feed-forward half live in registers and in the wave's own LDS.
//
// Arithmetic: exact-f32 matrix cores (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain) for the four dense
// products (q/k/v, output projection, the two feed-forward layers), f32 vector ALU for the layer norms, the 6 x 6 scores,
// the softmax (max-subtracted, v_exp_f32) and the context.  Layer norm, dense chain, feed-forward half, tile load and
// store and the weight view are jg_mixer_dev.h's; this file holds the tile, the LDS map and the 6 x 6 attention.
//
// Weights (12 288 floats at C 32 / F 128, 49 152 at C 64 / F 256 - more than a CU's LDS at the wider size) are not staged:
// a B operand is one coalesced 256-byte read of the packed blob per 4 x 16 slab, reused by the six token blocks, and every
// wave of the launch reads the same few kilobytes - they stay in L2.
//
// LDS of a wave (= a workgroup of 64 threads, so a barrier is a wave's own): xn[96][C + 2] (LN output / the A operand of
// the products that read the tokens) and qb[96][3 G + 2] (q | k | v of one group of G = max(16, D) channels, later the
// group's context in q's place, later 16 hidden columns of the feed-forward half).  Row pitches = 2 mod 4
// (jg_mixer_dev.h).
#include "jg_common.h"
#include "jg_frameattn.h"
#include "jg_mixer_dev.h"

namespace {

template <int C>
__global__ __launch_bounds__(64) void frameattn_kernel(JgFrameAttnArgs a) {
  extern __shared__ float fa_lds[];
  constexpr int NB = C / 16, SX = C + 2;
  const int D = a.D, F = a.F;
  const int G = D > 16 ? D : 16, SQ = 3 * G + 2;
  float *xn = fa_lds, *qb = fa_lds + 96 * SX;
  const int lane = threadIdx.x, n = lane & 15, j = lane >> 4;
  const int win = blockIdx.x / a.tiles, p0 = (blockIdx.x - win * a.tiles) * 16;
  const int L = a.L;
  const JgAttnWeights w = jg_attn_weights(a.w, C, F);

  // ---- the tile: block f = frame f, rows = positions p0 .. p0 + 15 (token t = frame t >> 4, position p0 + (t & 15));
  // rows past the end of the frame are zeros, never stored.  The residual stream stays in xr to the store.
  f32x4 xr[6][NB];
  const auto pos = [=](int t) { return p0 + (t & 15); };
  const auto in_frame = [=](int t) { return pos(t) < L; };
  const float *__restrict__ xw = a.x + (size_t)win * 6 * L * C;
  jg_mixer_load_tile<C, SX, 64>(xn, 96, lane, in_frame, [=](int t) { return xw + ((size_t)(t >> 4) * L + pos(t)) * C; });
  __syncthreads();
  jg_mixer_get<C, 6>(xr, xn, n, j);
  __syncthreads();
  jg_mixer_layernorm<C, 64>(xn, 96, lane, a.eps);
  jg_mixer_add_bias<C, 6>(xr, w.bo, n);
  __syncthreads();

  // ---- attention, a group of G channels (16 / D heads, or one head of D >= 16 channels) at a time
  for (int g0 = 0; g0 < C; g0 += G) {
    for (int which = 0; which < 3; ++which)
      for (int gb = 0; gb < G; gb += 16) {
        const int col = g0 + gb + n;
        f32x4 acc[6];
        const float bias = w.bqkv[which * C + col];
#pragma unroll
        for (int f = 0; f < 6; ++f) acc[f] = f32x4{bias, bias, bias, bias};
        jg_mixer_dense<6, C>(xn, SX, w.wqkv + (size_t)which * C * C + col, C, acc, n, j);
#pragma unroll
        for (int f = 0; f < 6; ++f)
#pragma unroll
          for (int i = 0; i < 4; ++i) qb[(f * 16 + 4 * j + i) * SQ + which * G + gb + n] = acc[f][i];
      }
    __syncthreads();
    // scores, softmax over the six keys, context: one lane per (position, head of the group)
    for (int pr = lane; pr < 16 * (G / D); pr += 64) {
      const int p = pr & 15, hc = (pr >> 4) * D;
      float s[6][6];
#pragma unroll
      for (int f = 0; f < 6; ++f)
#pragma unroll
        for (int g = 0; g < 6; ++g) s[f][g] = 0.f;
      for (int d = 0; d < D; ++d) {
        float q[6], k[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          q[f] = qb[(f * 16 + p) * SQ + hc + d];
          k[f] = qb[(f * 16 + p) * SQ + G + hc + d];
        }
#pragma unroll
        for (int f = 0; f < 6; ++f)
#pragma unroll
          for (int g = 0; g < 6; ++g) s[f][g] = fmaf(q[f], k[g], s[f][g]);
      }
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        float mx = s[f][0];
#pragma unroll
        for (int g = 1; g < 6; ++g) mx = fmaxf(mx, s[f][g]);
        float sum = 0.f;
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          s[f][g] = __builtin_amdgcn_exp2f((s[f][g] - mx) * 1.44269504f);
          sum += s[f][g];
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int g = 0; g < 6; ++g) s[f][g] *= inv;
      }
      for (int d = 0; d < D; ++d) {
        float v[6];
#pragma unroll
        for (int g = 0; g < 6; ++g) v[g] = qb[(g * 16 + p) * SQ + 2 * G + hc + d];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          float c = s[f][0] * v[0];
#pragma unroll
          for (int g = 1; g < 6; ++g) c = fmaf(s[f][g], v[g], c);
          qb[(f * 16 + p) * SQ + hc + d] = c;          // the context takes the query's place (this lane alone read it)
        }
      }
    }
    __syncthreads();
    // output projection of the group's context onto the residual stream
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float *__restrict__ wcol = w.wo + (size_t)g0 * C + nb * 16 + n;
#pragma unroll 4
      for (int k0 = 0; k0 < G; k0 += 4) {
        const float b = wcol[(k0 + j) * C];
#pragma unroll
        for (int f = 0; f < 6; ++f)
          xr[f][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qb[(f * 16 + n) * SQ + k0 + j], b, xr[f][nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- feed-forward half, 16 hidden columns at a time
  if (F > 0) jg_attn_ffn<C, 6, 64>(xr, xn, 96, xn, qb, w, F, a.eps, lane, n, j);

  // ---- store, with the stages the compiler fused behind the layer
  jg_mixer_put<C, 6>(xn, xr, n, j);
  __syncthreads();
  float *__restrict__ yw = a.y + (size_t)win * 6 * L * C;
  jg_mixer_store_tile<C, 64>(xn, 96, lane, a.st, a.n_stages, in_frame, [=](int t) { return yw + ((size_t)(t >> 4) * L + pos(t)) * C; });
}

int64_t lds_bytes(int C, int D, int F) {
  const int G = D > 16 ? D : 16;
  (void)F;                                          // (the 96 x 18 hidden columns fit q | k | v's place: 3 G + 2 >= 50)
  return (int64_t)96 * ((C + 2) + (3 * G + 2)) * (int64_t)sizeof(float);
}

}  // namespace

bool jg_frameattn_supports(int C, int H, int F, char *why, size_t cap) { return jg_attn_supports(false, true, C, H, F, why, cap); }

int64_t jg_frameattn_blob_floats(int C, int F) { return jg_attn_blob_floats(C, F); }

int jg_launch_frameattn(jg_engine *e, const JgFrameAttnArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_frameattn_supports(a.C, a.H, a.F, why, sizeof(why)), JG_ERR_UNSUPPORTED, "frame attention: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.n_win >= 1 && a.L >= 1 && a.D * a.H == a.C &&
                 a.tiles == (a.L + 15) / 16 && (int64_t)a.n_win * a.tiles <= 0x7fffffff,
             JG_ERR_INVALID, "frame attention: bad launch arguments");
  const int64_t lds = lds_bytes(a.C, a.D, a.F);
  JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "frame attention: %lld bytes of LDS", (long long)lds);
  static int64_t opened[2] = {0, 0};
  const int64_t grid = (int64_t)a.n_win * a.tiles;
  return a.C == 32 ? jg_mixer_launch(frameattn_kernel<32>, opened[0], grid, 64, lds, s, a)
                   : jg_mixer_launch(frameattn_kernel<64>, opened[1], grid, 64, lds, s, a);
}
