// One block of LocalAttention (reference: nnlib/v2/layers.py:2520-2645) as ONE launch: inside every frame row the
// positions are tokens of C channels and a query attends the keys at most `half` = window_size // 2 positions away -
//   x_norm = LayerNormalization(eps 1e-6)(x)                                              :2556-2558, :2612
//   x      = x + MultiHeadAttention(H heads, key_dim D = C / H)(x_norm, x_norm, attention_mask = M)   :2559-2564, :2613-2619
//   x      = x + Dense(C)(gelu(Dense(F)(LayerNormalization(eps 1e-6)(x))))                :2565-2575, :2621-2623
// with M[q, k] = (|q - k| <= half) and mask[k] (:2579-2585, :2604-2609).  The dense phases are the shared code of
// jg_mixer_dev.h on the exact-f32 matrix cores; this file holds where the tokens lie and the banded attention:
//
// A wave owns a tile of T = 80 consecutive query positions of one row (five 16-row blocks of the matrix cores) plus a halo
// of HB = ceil(half / 16) whole blocks on each side.  Layer norm, k and v are computed for tile + halo, q, the context, the
// projection and the feed-forward half for the 80 queries.  Halo tokens in front of position 0 or at / behind L are not
// keys: they are zero-filled and marked invalid, never read from the neighbouring row's memory.  Key validity otherwise
// comes from the mask bytes of the row, loaded with the tile.  Scores, softmax and context of a (query, head) run on the
// vector ALUs over the up to 2 half + 1 keys of the band out of LDS; a masked key is skipped (Keras adds -1e9 to its score:
// its exp is exactly 0 wherever the row has a valid key).  A query whose band holds no valid key (a "dead" position: Keras'
// value there depends on its version and precision) stores exact zeros, behind the fused stages too.
//
// The op is out of place by construction: a neighbouring tile reads this tile's positions as its halo.
//
// LDS of a wave (= a workgroup of 64 threads): xn[NTOK][C + 2] (LN output, the A operand), qb[NTOK][3 G + 2] (q | k | v of
// one group of G = max(16, D) channels, the context in q's place, later 16 hidden columns), valid[NTOK], dead[80] and the
// probabilities sc[64][2 half + 1] of the (query, head) pairs in flight - in xn's place where one group covers all
// channels (xn is then not read again before the feed-forward half rewrites it) and the rows fit.
#include "jg_common.h"
#include "jg_localattn.h"
#include "jg_mixer_dev.h"

namespace {

constexpr int T = JG_LOCALATTN_TILE, QB = T / 16;

__host__ __device__ inline int la_group(int D) { return D > 16 ? D : 16; }
// the probabilities take xn's place when one group covers all channels and 64 rows of 2 half + 1 fit into xn
__host__ __device__ inline bool la_sc_in_xn(int C, int D, int half, int ntok) {
  return la_group(D) == C && ntok * (C + 2) >= 64 * (2 * half + 1);
}

template <int C, int HB>
__global__ __launch_bounds__(64) void localattn_kernel(JgLocalAttnArgs a) {
  extern __shared__ float la_lds[];
  constexpr int NB = C / 16, SX = C + 2, NT = QB + 2 * HB, NTOK = NT * 16, HALO = HB * 16;
  const int D = a.D, F = a.F, half = a.half, SP = 2 * half + 1;
  const int G = la_group(D), SQ = 3 * G + 2;
  float *xn = la_lds, *qb = la_lds + NTOK * SX;
  int *valid = reinterpret_cast<int *>(qb + NTOK * SQ), *dead = valid + NTOK;
  float *sc = la_sc_in_xn(C, D, half, NTOK) ? xn : reinterpret_cast<float *>(dead + T);
  const int lane = threadIdx.x, n = lane & 15, j = lane >> 4;
  const int row = blockIdx.x / a.tiles, p0 = (blockIdx.x - row * a.tiles) * T;
  const int L = a.L;
  const JgAttnWeights w = jg_attn_weights(a.w, C, F);

  // ---- tile + halo: token t = position p0 - HALO + t of this row; positions outside [0, L) are zero rows and no keys
  // (the bytes in front of the row / behind it belong to the neighbouring rows: never read)
  const float *__restrict__ xrow = a.x + (size_t)row * L * C;
  jg_mixer_load_tile<C, SX, 64>(xn, NTOK, lane, [=](int t) { return p0 - HALO + t >= 0 && p0 - HALO + t < L; },
                                [=](int t) { return xrow + (size_t)(p0 - HALO + t) * C; });
  for (int t = lane; t < NTOK; t += 64) {
    const int p = p0 - HALO + t;
    int ok = p >= 0 && p < L;
    if (ok && a.mask != nullptr) ok = a.mask[(size_t)row * L + p] != 0;
    valid[t] = ok;
  }
  __syncthreads();
  for (int p = lane; p < T; p += 64) {                       // (HALO >= half: the band stays inside the NTOK tokens)
    int any = 0;
    for (int dj = -half; dj <= half; ++dj) any |= valid[HALO + p + dj];
    dead[p] = !any;
  }
  // the residual stream of the 80 queries: accumulator layout (column = lane & 15 = channel, row = 4 (lane >> 4) +
  // register = position), in these registers to the store
  f32x4 xr[QB][NB];
  jg_mixer_get<C, QB>(xr, xn + HALO * SX, n, j);
  __syncthreads();
  jg_mixer_layernorm<C, 64>(xn, NTOK, lane, a.eps);
  // (x + b_o written out, not jg_mixer_add_bias: through the helper the compiler schedules this kernel 7.6 % slower -
  // 8.70 ms against 8.08 ms per launch of localattn500's block at 3072 windows)
#pragma unroll
  for (int f = 0; f < QB; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float b = w.bo[nb * 16 + n];
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] += b;
    }
  __syncthreads();

  // ---- attention, a group of G channels (16 / D heads, or one head of D >= 16 channels) at a time
  for (int g0 = 0; g0 < C; g0 += G) {
    for (int gb = 0; gb < G; gb += 16) {
      const int col = g0 + gb + n;
      {                                                      // q: the 80 queries
        f32x4 acc[QB];
        const float bias = w.bqkv[col];
#pragma unroll
        for (int f = 0; f < QB; ++f) acc[f] = f32x4{bias, bias, bias, bias};
        jg_mixer_dense<QB, C>(xn + HALO * SX, SX, w.wqkv + col, C, acc, n, j);
#pragma unroll
        for (int f = 0; f < QB; ++f)
#pragma unroll
          for (int i = 0; i < 4; ++i) qb[(HALO + f * 16 + 4 * j + i) * SQ + gb + n] = acc[f][i];
      }
      for (int which = 1; which < 3; ++which) {              // k, v: tile + halo
        f32x4 acc[NT];
        const float bias = w.bqkv[which * C + col];
#pragma unroll
        for (int f = 0; f < NT; ++f) acc[f] = f32x4{bias, bias, bias, bias};
        jg_mixer_dense<NT, C>(xn, SX, w.wqkv + (size_t)which * C * C + col, C, acc, n, j);
#pragma unroll
        for (int f = 0; f < NT; ++f)
#pragma unroll
          for (int i = 0; i < 4; ++i) qb[(f * 16 + 4 * j + i) * SQ + which * G + gb + n] = acc[f][i];
      }
    }
    __syncthreads();
    // scores, softmax over the valid keys of the band, context: one lane per (query, head of the group)
    for (int it = lane; it < T * (G / D); it += 64) {
      const int p = it % T, hc = (it / T) * D, tq = HALO + p;
      float *qrow = qb + tq * SQ + hc;
      float *srow = sc + lane * SP;
      float mx = -INFINITY;
      for (int dj = 0; dj < SP; ++dj) {
        const int t = tq - half + dj;
        if (!valid[t]) continue;
        const float *krow = qb + t * SQ + G + hc;
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(qrow[d], krow[d], s);
        srow[dj] = s;
        mx = fmaxf(mx, s);
      }
      float sum = 0.f;
      for (int dj = 0; dj < SP; ++dj) {
        if (!valid[tq - half + dj]) continue;
        const float e = __builtin_amdgcn_exp2f((srow[dj] - mx) * 1.44269504f);
        srow[dj] = e;
        sum += e;
      }
      const float inv = sum > 0.f ? 1.0f / sum : 0.f;        // (no valid key: a dead query, zeroed at the store)
      for (int d = 0; d < D; ++d) {
        float c = 0.f;
        for (int dj = 0; dj < SP; ++dj) {
          const int t = tq - half + dj;
          if (valid[t]) c = fmaf(srow[dj], qb[t * SQ + 2 * G + hc + d], c);
        }
        qrow[d] = c * inv;                                   // the context takes the query's place (this lane alone read it)
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
        for (int f = 0; f < QB; ++f)
          xr[f][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qb[(HALO + f * 16 + n) * SQ + k0 + j], b, xr[f][nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- feed-forward half on the 80 queries (rows 0 .. 79 of xn and qb from here on)
  jg_attn_ffn<C, QB, 64>(xr, xn, T, xn, qb, w, F, a.eps, lane, n, j);

  // ---- store, with the stages the compiler fused behind the block: jg_mixer_store_tile with one rule more - dead
  // positions are exact zeros, behind the stages too.  (Written out here: with the rule as a third predicate of the shared
  // store the compiler spends 8 more registers on the 16-channel, no-halo instantiation.)
  jg_mixer_put<C, QB>(xn, xr, n, j);
  __syncthreads();
  float *__restrict__ yrow = a.y + (size_t)row * L * C;
  for (int q = lane; q < T * (C / 4); q += 64) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4, p = p0 + t;
    if (p >= L) continue;
    const float *r = xn + t * SX + c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!dead[t]) {
      v.x = jg_mixer_stages(r[0], a.st, a.n_stages, c4);
      v.y = jg_mixer_stages(r[1], a.st, a.n_stages, c4 + 1);
      v.z = jg_mixer_stages(r[2], a.st, a.n_stages, c4 + 2);
      v.w = jg_mixer_stages(r[3], a.st, a.n_stages, c4 + 3);
    }
    *reinterpret_cast<float4 *>(yrow + (size_t)p * C + c4) = v;
  }
}

template <int C>
int launch_c(const JgLocalAttnArgs &a, int hb, int64_t lds, hipStream_t s) {
  auto kern = hb == 0 ? localattn_kernel<C, 0> : hb == 1 ? localattn_kernel<C, 1> : localattn_kernel<C, 2>;
  static int64_t opened[3] = {0, 0, 0};
  return jg_mixer_launch(kern, opened[hb], (int64_t)a.rows * a.tiles, 64, lds, s, a);
}

}  // namespace

bool jg_localattn_supports(int C, int H, int F, int half, char *why, size_t cap) {
  if (!jg_attn_supports(true, false, C, H, F, why, cap)) return false;
  if (half < 0 || half > JG_LOCALATTN_MAX_HALF) {
    snprintf(why, cap, "half-window %d (0 to %d positions on each side)", half, JG_LOCALATTN_MAX_HALF);
    return false;
  }
  return true;
}

int64_t jg_localattn_blob_floats(int C, int F) { return jg_attn_blob_floats(C, F); }

int64_t jg_localattn_lds_bytes(int C, int D, int half) {
  const int ntok = (QB + 2 * ((half + 15) / 16)) * 16, G = la_group(D);
  // (the 80 x 18 hidden columns fit q | k | v's place: 3 G + 2 >= 50)
  return ((int64_t)ntok * ((C + 2) + (3 * G + 2)) + ntok + T + (la_sc_in_xn(C, D, half, ntok) ? 0 : 64 * (2 * half + 1))) *
         (int64_t)sizeof(float);
}

int jg_launch_localattn(jg_engine *e, const JgLocalAttnArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_localattn_supports(a.C, a.H, a.F, a.half, why, sizeof(why)), JG_ERR_UNSUPPORTED, "local attention: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.rows >= 1 && a.L >= 1 && a.D * a.H == a.C &&
                 a.tiles == (a.L + T - 1) / T && (int64_t)a.rows * a.tiles <= 0x7fffffff,
             JG_ERR_INVALID, "local attention: bad launch arguments");
  JG_REQUIRE(a.y != a.x, JG_ERR_INVALID, "local attention: the op cannot run in place (a tile reads its neighbours' positions as its halo)");
  const int64_t lds = jg_localattn_lds_bytes(a.C, a.D, a.half);
  JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "local attention: %lld bytes of LDS", (long long)lds);
  const int hb = (a.half + 15) / 16;
  return a.C == 16 ? launch_c<16>(a, hb, lds, s) : a.C == 32 ? launch_c<32>(a, hb, lds, s) : launch_c<64>(a, hb, lds, s);
}
