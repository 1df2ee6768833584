// One block of LocalAttention (reference: nnlib/v2/layers.py:2520-2645) as ONE launch: inside every frame row the
// positions are tokens of C channels and a query attends the keys at most `half` = window_size // 2 positions away -
//   x_norm = LayerNormalization(eps 1e-6)(x)                                              :2556-2558, :2612
//   x      = x + MultiHeadAttention(H heads, key_dim D = C / H)(x_norm, x_norm, attention_mask = M)   :2559-2564, :2613-2619
//   x      = x + Dense(C)(gelu(Dense(F)(LayerNormalization(eps 1e-6)(x))))                :2565-2575, :2621-2623
// with M[q, k] = (|q - k| <= half) and mask[k] (:2579-2585, :2604-2609).  The dense phases are the mathematics of the
// frame-attention kernel (jg_frameattn.hip) on the same exact-f32 matrix cores; what differs is where the tokens lie:
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

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int T = JG_LOCALATTN_TILE, QB = T / 16;

// the activations of jg_kernels.hip: jg_apply_act (tanh-GELU and sigmoid through v_exp_f32 / v_rcp_f32)
__device__ __forceinline__ float la_act(float v, int act) {
  switch (act) {
    case JG_ACT_GELU_TANH: {
      const float t = v * (-2.3022082f - 0.10294324f * v * v);   // -2u * log2(e), u = sqrt(2/pi)(x + 0.044715 x^3)
      return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
    }
    case JG_ACT_GELU_ERF: return 0.5f * v * erfcf(-v * 0.70710678118654752f);
    case JG_ACT_RELU: return fmaxf(v, 0.0f);
    case JG_ACT_TANH: return tanhf(v);
    case JG_ACT_SIGMOID: return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950f * v));
    default: return v;
  }
}

// the op's stage list on one element of channel c (validate_program refuses the stages that need a mask, another tensor
// or a reduction behind this op)
__device__ __forceinline__ float la_stages(float v, const StageArg *st, int n_stages, int c) {
  for (int s = 0; s < n_stages; ++s) {
    const StageArg &g = st[s];
    switch (g.kind) {
      case JG_ST_BIAS: v += g.p0[c]; break;
      case JG_ST_BN: v = g.p2[c] * ((v - g.p0[c]) * g.p1[c]) + g.p3[c]; break;
      case JG_ST_DYT: v = tanhf(g.f0 * v) * g.p2[c] + g.p3[c]; break;
      case JG_ST_ACT: v = la_act(v, g.arg); break;
      default: break;
    }
  }
  return v;
}

// LayerNormalization without gamma / beta (folded into the next kernel), in place on `rows` token rows of xn: biased
// variance of the centred values, 1 / sqrt(var + eps)
template <int C>
__device__ __forceinline__ void la_layernorm(float *xn, int rows, int lane, float eps) {
  constexpr int SX = C + 2;
  for (int t = lane; t < rows; t += 64) {
    float *row = xn + t * SX;
    float sum = 0.f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) sum += row[c];
    const float mean = sum * (1.0f / C);
    float sq = 0.f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
      const float d = row[c] - mean;
      sq = fmaf(d, d, sq);
    }
    const float rstd = 1.0f / sqrtf(sq * (1.0f / C) + eps);
#pragma unroll 8
    for (int c = 0; c < C; ++c) row[c] = (row[c] - mean) * rstd;
  }
}

// acc[f] += A[block f] (16 x K, rows `lda` apart in LDS) @ B (K x 16 columns of a row-major matrix, `ldw` floats a row):
// a k-ordered fmaf chain per element on the exact-f32 matrix cores; one B read serves the NBLK token blocks
template <int NBLK, int K>
__device__ __forceinline__ void la_dense(const float *a_rows, int lda, const float *__restrict__ wcol, int ldw,
                                         f32x4 (&acc)[NBLK], int n, int j) {
#pragma unroll
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float b = wcol[(size_t)(k0 + j) * ldw];
#pragma unroll
    for (int f = 0; f < NBLK; ++f)
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_rows[(f * 16 + n) * lda + k0 + j], b, acc[f], 0, 0, 0);
  }
}

__host__ __device__ inline int la_group(int D) { return D > 16 ? D : 16; }
// the probabilities take xn's place when one group covers all channels and 64 rows of 2 half + 1 fit into xn
__host__ __device__ inline bool la_sc_in_xn(int C, int D, int half, int ntok) {
  return la_group(D) == C && ntok * (C + 2) >= 64 * (2 * half + 1);
}

template <int C, int HB>
__global__ __launch_bounds__(64) void localattn_kernel(JgLocalAttnArgs a) {
  extern __shared__ float la_lds[];
  constexpr int NB = C / 16, SX = C + 2, SH = 18, NT = QB + 2 * HB, NTOK = NT * 16, HALO = HB * 16;
  const int D = a.D, F = a.F, half = a.half, SP = 2 * half + 1;
  const int G = la_group(D), SQ = 3 * G + 2;
  float *xn = la_lds, *qb = la_lds + NTOK * SX;
  int *valid = reinterpret_cast<int *>(qb + NTOK * SQ), *dead = valid + NTOK;
  float *sc = la_sc_in_xn(C, D, half, NTOK) ? xn : reinterpret_cast<float *>(dead + T);
  const int lane = threadIdx.x, n = lane & 15, j = lane >> 4;
  const int row = blockIdx.x / a.tiles, p0 = (blockIdx.x - row * a.tiles) * T;
  const int L = a.L;
  // packed weights (program.py: pack_local_attn - the frame-attention layout)
  const float *__restrict__ wqkv = a.w;                       // [3][C][C]   (q | k | v, input channel, h D + d)
  const float *__restrict__ bqkv = wqkv + 3 * C * C;          // [3][C]
  const float *__restrict__ wo = bqkv + 3 * C;                // [C][C]      (h D + d, output channel)
  const float *__restrict__ bo = wo + C * C;                  // [C]
  const float *__restrict__ w1 = bo + C;                      // [C][F]
  const float *__restrict__ b1 = w1 + C * F;                  // [F]
  const float *__restrict__ w2 = b1 + F;                      // [F][C]
  const float *__restrict__ b2 = w2 + F * C;                  // [C]

  // ---- tile + halo: token t = position p0 - HALO + t of this row; positions outside [0, L) are zero rows and no keys
  // (the bytes in front of the row / behind it belong to the neighbouring rows: never read)
  const float *__restrict__ xrow = a.x + (size_t)row * L * C;
  for (int q = lane; q < NTOK * (C / 4); q += 64) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4, p = p0 - HALO + t;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p >= 0 && p < L) v = *reinterpret_cast<const float4 *>(xrow + (size_t)p * C + c4);
    float *r = xn + t * SX + c4;
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  }
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
#pragma unroll
  for (int f = 0; f < QB; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] = xn[(HALO + f * 16 + 4 * j + i) * SX + nb * 16 + n];
  __syncthreads();
  la_layernorm<C>(xn, NTOK, lane, a.eps);
#pragma unroll
  for (int f = 0; f < QB; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float b = bo[nb * 16 + n];
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
        const float bias = bqkv[col];
#pragma unroll
        for (int f = 0; f < QB; ++f) acc[f] = f32x4{bias, bias, bias, bias};
        la_dense<QB, C>(xn + HALO * SX, SX, wqkv + col, C, acc, n, j);
#pragma unroll
        for (int f = 0; f < QB; ++f)
#pragma unroll
          for (int i = 0; i < 4; ++i) qb[(HALO + f * 16 + 4 * j + i) * SQ + gb + n] = acc[f][i];
      }
      for (int which = 1; which < 3; ++which) {              // k, v: tile + halo
        f32x4 acc[NT];
        const float bias = bqkv[which * C + col];
#pragma unroll
        for (int f = 0; f < NT; ++f) acc[f] = f32x4{bias, bias, bias, bias};
        la_dense<NT, C>(xn, SX, wqkv + (size_t)which * C * C + col, C, acc, n, j);
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
      const float *__restrict__ wcol = wo + (size_t)g0 * C + nb * 16 + n;
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

  // ---- feed-forward half on the 80 queries (rows 0 .. 79 of xn and qb from here on), 16 hidden columns at a time
#pragma unroll
  for (int f = 0; f < QB; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) xn[(f * 16 + 4 * j + i) * SX + nb * 16 + n] = xr[f][nb][i];
  __syncthreads();
  la_layernorm<C>(xn, T, lane, a.eps);
#pragma unroll
  for (int f = 0; f < QB; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float b = b2[nb * 16 + n];
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] += b;
    }
  __syncthreads();
  for (int hb = 0; hb < F; hb += 16) {
    f32x4 acc[QB];
    const float bias = b1[hb + n];
#pragma unroll
    for (int f = 0; f < QB; ++f) acc[f] = f32x4{bias, bias, bias, bias};
    la_dense<QB, C>(xn, SX, w1 + hb + n, F, acc, n, j);
#pragma unroll
    for (int f = 0; f < QB; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) qb[(f * 16 + 4 * j + i) * SH + n] = la_act(acc[f][i], JG_ACT_GELU_TANH);
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float *__restrict__ w2col = w2 + (size_t)hb * C + nb * 16 + n;
#pragma unroll
      for (int k0 = 0; k0 < 16; k0 += 4) {
        const float b = w2col[(k0 + j) * C];
#pragma unroll
        for (int f = 0; f < QB; ++f)
          xr[f][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qb[(f * 16 + n) * SH + k0 + j], b, xr[f][nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- store, with the stages the compiler fused behind the block: through LDS again, so that a lane quad writes 16
  // consecutive bytes of a token row; positions at / behind L are not written, dead positions are exact zeros
#pragma unroll
  for (int f = 0; f < QB; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) xn[(f * 16 + 4 * j + i) * SX + nb * 16 + n] = xr[f][nb][i];
  __syncthreads();
  float *__restrict__ yrow = a.y + (size_t)row * L * C;
  for (int q = lane; q < T * (C / 4); q += 64) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4, p = p0 + t;
    if (p >= L) continue;
    const float *r = xn + t * SX + c4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!dead[t]) {
      v.x = la_stages(r[0], a.st, a.n_stages, c4);
      v.y = la_stages(r[1], a.st, a.n_stages, c4 + 1);
      v.z = la_stages(r[2], a.st, a.n_stages, c4 + 2);
      v.w = la_stages(r[3], a.st, a.n_stages, c4 + 3);
    }
    *reinterpret_cast<float4 *>(yrow + (size_t)p * C + c4) = v;
  }
}

template <int C>
int launch_c(const JgLocalAttnArgs &a, int hb, int64_t lds, hipStream_t s) {
  auto kern = hb == 0 ? localattn_kernel<C, 0> : hb == 1 ? localattn_kernel<C, 1> : localattn_kernel<C, 2>;
  static int64_t attr_set[3] = {0, 0, 0};           // largest dynamic-LDS size each instantiation was opened for
  if (lds > attr_set[hb]) {
    JG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set[hb] = lds;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)a.rows * a.tiles)), dim3(64), (size_t)lds, s, a);
  JG_HIP(hipGetLastError());
  return JG_OK;
}

}  // namespace

bool jg_localattn_supports(int C, int H, int F, int half, char *why, size_t cap) {
  if (C != 16 && C != 32 && C != 64) {
    snprintf(why, cap, "%d channels (the kernel covers 16, 32 and 64)", C);
    return false;
  }
  const int D = H >= 1 && C % H == 0 ? C / H : 0;
  if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) {
    snprintf(why, cap, "%d heads at %d channels (key_dim = channels / heads must be 4, 8, 16, 32 or 64)", H, C);
    return false;
  }
  if (F % 16 != 0 || F < 16 || F > 256) {
    snprintf(why, cap, "feed-forward width %d (a multiple of 16 up to 256)", F);
    return false;
  }
  if (half < 0 || half > JG_LOCALATTN_MAX_HALF) {
    snprintf(why, cap, "half-window %d (0 to %d positions on each side)", half, JG_LOCALATTN_MAX_HALF);
    return false;
  }
  return true;
}

int64_t jg_localattn_blob_floats(int C, int F) { return (int64_t)4 * C * C + 4 * C + (int64_t)2 * C * F + F + C; }

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
