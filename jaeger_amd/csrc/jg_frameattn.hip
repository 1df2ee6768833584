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
// the softmax (max-subtracted, v_exp_f32) and the context.  The host folds the layer norms' gamma / beta into the kernels
// and biases that follow them and 1 / sqrt(D) into the query (program.py: pack_frame_attn, float64).
//
// Weights (12 288 floats at C 32 / F 128, 49 152 at C 64 / F 256 - more than a CU's LDS at the wider size) are not staged:
// a B operand is one coalesced 256-byte read of the packed blob per 4 x 16 slab, reused by the six token blocks, and every
// wave of the launch reads the same few kilobytes - they stay in L2.
//
// LDS of a wave (= a workgroup of 64 threads, so a barrier is a wave's own): xn[96][C + 2] (LN output / the A operand of
// the products that read the tokens) and qb[96][3 G + 2] (q | k | v of one group of G = max(16, D) channels, later the
// group's context in q's place, later 16 hidden columns of the feed-forward half).  Row pitches = 2 mod 4: the A-operand
// reads (row = lane & 15, column = k0 + (lane >> 4)) of a 32-lane half hit 32 different banks.
#include "jg_common.h"
#include "jg_frameattn.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// the activations of jg_kernels.hip: jg_apply_act (tanh-GELU and sigmoid through v_exp_f32 / v_rcp_f32)
__device__ __forceinline__ float fa_act(float v, int act) {
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

// the op's stage list on one element of channel c (the stages of jg_kernels.hip: jg_apply_stages that need no mask, no
// other tensor and no reduction - validate_program refuses the others behind this op)
__device__ __forceinline__ float fa_stages(float v, const StageArg *st, int n_stages, int c) {
  for (int s = 0; s < n_stages; ++s) {
    const StageArg &g = st[s];
    switch (g.kind) {
      case JG_ST_BIAS: v += g.p0[c]; break;
      case JG_ST_BN: v = g.p2[c] * ((v - g.p0[c]) * g.p1[c]) + g.p3[c]; break;
      case JG_ST_DYT: v = tanhf(g.f0 * v) * g.p2[c] + g.p3[c]; break;
      case JG_ST_ACT: v = fa_act(v, g.arg); break;
      default: break;
    }
  }
  return v;
}

// LayerNormalization without gamma / beta (folded into the next kernel), in place on the 96 token rows of xn: biased
// variance of the centred values, 1 / sqrt(var + eps)
template <int C>
__device__ __forceinline__ void fa_layernorm(float *xn, int lane, float eps) {
  constexpr int SX = C + 2;
  for (int t = lane; t < 96; t += 64) {
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

template <int C>
__global__ __launch_bounds__(64) void frameattn_kernel(JgFrameAttnArgs a) {
  extern __shared__ float fa_lds[];
  constexpr int NB = C / 16, SX = C + 2, SH = 18;
  const int D = a.D, F = a.F;
  const int G = D > 16 ? D : 16, SQ = 3 * G + 2;
  float *xn = fa_lds, *qb = fa_lds + 96 * SX;
  const int lane = threadIdx.x, n = lane & 15, j = lane >> 4;
  const int win = blockIdx.x / a.tiles, p0 = (blockIdx.x - win * a.tiles) * 16;
  const int L = a.L;
  // packed weights (program.py: pack_frame_attn)
  const float *__restrict__ wqkv = a.w;                       // [3][C][C]   (q | k | v, input channel, h D + d)
  const float *__restrict__ bqkv = wqkv + 3 * C * C;          // [3][C]
  const float *__restrict__ wo = bqkv + 3 * C;                // [C][C]      (h D + d, output channel)
  const float *__restrict__ bo = wo + C * C;                  // [C]
  const float *__restrict__ w1 = bo + C;                      // [C][F]
  const float *__restrict__ b1 = w1 + C * F;                  // [F]
  const float *__restrict__ w2 = b1 + F;                      // [F][C]
  const float *__restrict__ b2 = w2 + F * C;                  // [C]

  // ---- the tile: block f = frame f, rows = positions p0 .. p0 + 15; accumulator layout (column = lane & 15 = channel,
  // row = 4 (lane >> 4) + register = position) - the residual stream stays in these registers to the store
  f32x4 xr[6][NB];
  const float *__restrict__ xw = a.x + (size_t)win * 6 * L * C;
  // (through LDS: a lane quad reads 16 consecutive bytes of a token row; rows past the end of the frame are zeros, never stored)
  for (int q = lane; q < 96 * (C / 4); q += 64) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4, p = p0 + (t & 15);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < L) v = *reinterpret_cast<const float4 *>(xw + ((size_t)(t >> 4) * L + p) * C + c4);
    float *row = xn + t * SX + c4;
    row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 6; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] = xn[(f * 16 + 4 * j + i) * SX + nb * 16 + n];
  __syncthreads();
  fa_layernorm<C>(xn, lane, a.eps);
#pragma unroll
  for (int f = 0; f < 6; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float b = bo[nb * 16 + n];
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] += b;
    }
  __syncthreads();

  // ---- attention, a group of G channels (16 / D heads, or one head of D >= 16 channels) at a time
  for (int g0 = 0; g0 < C; g0 += G) {
    for (int which = 0; which < 3; ++which)
      for (int gb = 0; gb < G; gb += 16) {
        const int col = g0 + gb + n;
        f32x4 acc[6];
        const float bias = bqkv[which * C + col];
#pragma unroll
        for (int f = 0; f < 6; ++f) acc[f] = f32x4{bias, bias, bias, bias};
        const float *__restrict__ wcol = wqkv + (size_t)which * C * C + col;
#pragma unroll
        for (int k0 = 0; k0 < C; k0 += 4) {
          const float b = wcol[(k0 + j) * C];
#pragma unroll
          for (int f = 0; f < 6; ++f)
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(xn[(f * 16 + n) * SX + k0 + j], b, acc[f], 0, 0, 0);
        }
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
      const float *__restrict__ wcol = wo + (size_t)g0 * C + nb * 16 + n;
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
  if (F > 0) {
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 4; ++i) xn[(f * 16 + 4 * j + i) * SX + nb * 16 + n] = xr[f][nb][i];
    __syncthreads();
    fa_layernorm<C>(xn, lane, a.eps);
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float b = b2[nb * 16 + n];
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[f][nb][i] += b;
      }
    __syncthreads();
    for (int hb = 0; hb < F; hb += 16) {
      f32x4 acc[6];
      const float bias = b1[hb + n];
#pragma unroll
      for (int f = 0; f < 6; ++f) acc[f] = f32x4{bias, bias, bias, bias};
      const float *__restrict__ wcol = w1 + hb + n;
#pragma unroll
      for (int k0 = 0; k0 < C; k0 += 4) {
        const float b = wcol[(size_t)(k0 + j) * F];
#pragma unroll
        for (int f = 0; f < 6; ++f)
          acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(xn[(f * 16 + n) * SX + k0 + j], b, acc[f], 0, 0, 0);
      }
#pragma unroll
      for (int f = 0; f < 6; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) qb[(f * 16 + 4 * j + i) * SH + n] = fa_act(acc[f][i], JG_ACT_GELU_TANH);
      __syncthreads();
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float *__restrict__ w2col = w2 + (size_t)hb * C + nb * 16 + n;
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4) {
          const float b = w2col[(k0 + j) * C];
#pragma unroll
          for (int f = 0; f < 6; ++f)
            xr[f][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qb[(f * 16 + n) * SH + k0 + j], b, xr[f][nb], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }

  // ---- store, with the stages the compiler fused behind the layer: through LDS again, so that a lane quad writes 16
  // consecutive bytes of a token row and the stage list is code once, not once per accumulator register
#pragma unroll
  for (int f = 0; f < 6; ++f)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) xn[(f * 16 + 4 * j + i) * SX + nb * 16 + n] = xr[f][nb][i];
  __syncthreads();
  float *__restrict__ yw = a.y + (size_t)win * 6 * L * C;
  for (int q = lane; q < 96 * (C / 4); q += 64) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4, p = p0 + (t & 15);
    if (p >= L) continue;
    const float *row = xn + t * SX + c4;
    float4 v;
    v.x = fa_stages(row[0], a.st, a.n_stages, c4);
    v.y = fa_stages(row[1], a.st, a.n_stages, c4 + 1);
    v.z = fa_stages(row[2], a.st, a.n_stages, c4 + 2);
    v.w = fa_stages(row[3], a.st, a.n_stages, c4 + 3);
    *reinterpret_cast<float4 *>(yw + ((size_t)(t >> 4) * L + p) * C + c4) = v;
  }
}

int64_t lds_bytes(int C, int D, int F) {
  const int G = D > 16 ? D : 16;
  (void)F;                                          // (the 96 x 18 hidden columns fit q | k | v's place: 3 G + 2 >= 50)
  return (int64_t)96 * ((C + 2) + (3 * G + 2)) * (int64_t)sizeof(float);
}

}  // namespace

bool jg_frameattn_supports(int C, int H, int F, char *why, size_t cap) {
  if (C != 32 && C != 64) {
    snprintf(why, cap, "%d channels (the kernel covers 32 and 64)", C);
    return false;
  }
  const int D = H >= 1 && C % H == 0 ? C / H : 0;
  if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) {
    snprintf(why, cap, "%d heads at %d channels (key_dim = channels / heads must be 4, 8, 16, 32 or 64)", H, C);
    return false;
  }
  if (F != 0 && (F % 16 != 0 || F < 16 || F > 256)) {
    snprintf(why, cap, "feed-forward width %d (0, or a multiple of 16 up to 256)", F);
    return false;
  }
  return true;
}

int64_t jg_frameattn_blob_floats(int C, int F) {
  return (int64_t)4 * C * C + 4 * C + (F > 0 ? (int64_t)2 * C * F + F + C : 0);
}

int jg_launch_frameattn(jg_engine *e, const JgFrameAttnArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_frameattn_supports(a.C, a.H, a.F, why, sizeof(why)), JG_ERR_UNSUPPORTED, "frame attention: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.n_win >= 1 && a.L >= 1 && a.D * a.H == a.C &&
                 a.tiles == (a.L + 15) / 16 && (int64_t)a.n_win * a.tiles <= 0x7fffffff,
             JG_ERR_INVALID, "frame attention: bad launch arguments");
  const int64_t lds = lds_bytes(a.C, a.D, a.F);
  JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "frame attention: %lld bytes of LDS", (long long)lds);
  auto kern = a.C == 32 ? frameattn_kernel<32> : frameattn_kernel<64>;
  static int64_t attr_set[2] = {0, 0};              // largest dynamic-LDS size each instantiation was opened for
  int64_t &have = attr_set[a.C == 32 ? 0 : 1];
  if (lds > have) {
    JG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    have = lds;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)a.n_win * a.tiles)), dim3(64), (size_t)lds, s, a);
  JG_HIP(hipGetLastError());
  return JG_OK;
}
