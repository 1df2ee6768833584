// What the row-mixer kernels (jg_frameattn.hip, jg_localattn.hip, jg_lengthattn.hip, jg_hyena.hip) share, written once:
// the element helpers (the activation - jg_kernels.hip takes it from here too - and the scalar stage tail), the tile
// helpers around the exact-f32 matrix cores, the attention ops' weight view and feed-forward half, and the host-side
// size checks and launch of the attention ops.  A kernel file keeps its tile geometry, its LDS map, which tokens are keys
// and its score / softmax / context loops.
//
// Conventions of every helper: a token row in LDS holds C channels at a pitch of C + 2 floats (= 2 mod 4: the A-operand
// reads - row = lane & 15, column = k0 + (lane >> 4) - of a 32-lane half hit 32 different banks); n = lane & 15 and
// j = lane >> 4 of the calling wave; a 16-row block of tokens is one block of the matrix cores, and its accumulator
// layout is column = n = channel, row = 4 j + register = token.
#pragma once
#include <math.h>
#include <stdio.h>

#include "jg_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- element helpers ---------------------------------------------------------------------------------------------------
// (tanh-GELU and sigmoid through v_exp_f32 / v_rcp_f32 - the formulas of the split-f16 kernels, jg_conv_dev.h -
// instead of libm's tanhf / expf: 8 instead of ~40 instructions per element; the exact-f32 conv's epilogue was a third
// of its tile time.  Saturates correctly: 2^t -> 0 or inf gives x or -0.)
__device__ __forceinline__ float jg_apply_act(float v, int act) {
  switch (act) {
    case JG_ACT_GELU_TANH: {
      // tf.nn.gelu(approximate=True): 0.5x(1+tanh(u)) = x / (1 + e^(-2u)), u = sqrt(2/pi)(x+0.044715x^3)
      const float t = v * (-2.3022082f - 0.10294324f * v * v);   // -2u * log2(e)
      return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
    }
    case JG_ACT_GELU_ERF:
      return 0.5f * v * erfcf(-v * 0.70710678118654752f);
    case JG_ACT_RELU:
      return fmaxf(v, 0.0f);
    case JG_ACT_TANH:
      // libm: 1 - 2 / (1 + e^(2v)) cancels for small |v| (relative error 1e-3 at |v| = 1e-4), and this kernel is the safe
      // path the range guard falls back to; a bare tanh activation is not on any hot path
      return tanhf(v);
    case JG_ACT_SIGMOID:
      return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950f * v));
    default:
      return v;
  }
}

// a row mixer's stage list on one element of channel c (the stages of jg_kernels.hip: jg_apply_stages that need no mask,
// no other tensor and no reduction - validate_program refuses the others behind these ops)
__device__ __forceinline__ float jg_mixer_stages(float v, const StageArg *st, int n_stages, int c) {
  for (int s = 0; s < n_stages; ++s) {
    const StageArg &g = st[s];
    switch (g.kind) {
      case JG_ST_BIAS: v += g.p0[c]; break;
      case JG_ST_BN: v = g.p2[c] * ((v - g.p0[c]) * g.p1[c]) + g.p3[c]; break;
      case JG_ST_DYT: v = tanhf(g.f0 * v) * g.p2[c] + g.p3[c]; break;
      case JG_ST_ACT: v = jg_apply_act(v, g.arg); break;
      default: break;
    }
  }
  return v;
}

// ---- tile helpers ------------------------------------------------------------------------------------------------------
// LayerNormalization without gamma / beta (folded into the next kernel), in place on `rows` token rows of xn, one of the
// workgroup's NTHREADS threads a row: biased variance of the centred values, 1 / sqrt(var + eps)
template <int C, int NTHREADS>
__device__ __forceinline__ void jg_mixer_layernorm(float *xn, int rows, int tid, float eps) {
  constexpr int SX = C + 2;
  for (int t = tid; t < rows; t += NTHREADS) {
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
// a k-ordered fmaf chain per element on the exact-f32 matrix cores (v_mfma_f32_16x16x4_f32); one B read serves the NBLK
// token blocks
template <int NBLK, int K>
__device__ __forceinline__ void jg_mixer_dense(const float *a_rows, int lda, const float *__restrict__ wcol, int ldw,
                                               f32x4 (&acc)[NBLK], int n, int j) {
#pragma unroll
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float b = wcol[(size_t)(k0 + j) * ldw];
#pragma unroll
    for (int f = 0; f < NBLK; ++f)
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_rows[(f * 16 + n) * lda + k0 + j], b, acc[f], 0, 0, 0);
  }
}

// the wave's NBLK token blocks x C channels between the LDS rows and registers in the accumulator layout
template <int C, int NBLK>
__device__ __forceinline__ void jg_mixer_get(f32x4 (&xr)[NBLK][C / 16], const float *rows, int n, int j) {
#pragma unroll
  for (int f = 0; f < NBLK; ++f)
#pragma unroll
    for (int nb = 0; nb < C / 16; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] = rows[(f * 16 + 4 * j + i) * (C + 2) + nb * 16 + n];
}
template <int C, int NBLK>
__device__ __forceinline__ void jg_mixer_put(float *rows, const f32x4 (&xr)[NBLK][C / 16], int n, int j) {
#pragma unroll
  for (int f = 0; f < NBLK; ++f)
#pragma unroll
    for (int nb = 0; nb < C / 16; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) rows[(f * 16 + 4 * j + i) * (C + 2) + nb * 16 + n] = xr[f][nb][i];
}

// a dense layer's bias onto the residual registers, ahead of the products that accumulate onto them
template <int C, int NBLK>
__device__ __forceinline__ void jg_mixer_add_bias(f32x4 (&xr)[NBLK][C / 16], const float *bias, int n) {
#pragma unroll
  for (int f = 0; f < NBLK; ++f)
#pragma unroll
    for (int nb = 0; nb < C / 16; ++nb) {
      const float b = bias[nb * 16 + n];
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[f][nb][i] += b;
    }
}

// `rows` tokens of C channels from global memory into LDS rows of pitch SD, a lane quad reading 16 consecutive bytes of
// a token.  Which tokens exist and where they lie is the caller's: in(t) says whether token t is read - any other is a
// zero row, its memory never touched - and at(t) gives the address of its C channels.  (Lambdas that capture by value:
// by reference the compiler spent two more scalar registers on hyena's projection kernel.)
template <int C, int SD, int NTHREADS, typename In, typename At>
__device__ __forceinline__ void jg_mixer_load_tile(float *dst, int rows, int tid, In in, At at) {
  for (int q = tid; q < rows * (C / 4); q += NTHREADS) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in(t)) v = *reinterpret_cast<const float4 *>(at(t) + c4);
    float *r = dst + t * SD + c4;
    if constexpr (SD % 4 == 0) {
      *reinterpret_cast<float4 *>(r) = v;
    } else {
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    }
  }
}

// the store of a mixer op: `rows` token rows of pitch C + 2 out of LDS, so that a lane quad writes 16 consecutive bytes
// of a token and the stage list is code once, not once per accumulator register.  in(t) and at(t) as above: a token
// that is not in is not written.
template <int C, int NTHREADS, typename In, typename At>
__device__ __forceinline__ void jg_mixer_store_tile(const float *src, int rows, int tid, const StageArg *st, int n_stages, In in, At at) {
  for (int q = tid; q < rows * (C / 4); q += NTHREADS) {
    const int t = q / (C / 4), c4 = (q - t * (C / 4)) * 4;
    if (!in(t)) continue;
    const float *r = src + t * (C + 2) + c4;
    float4 v;
    v.x = jg_mixer_stages(r[0], st, n_stages, c4);
    v.y = jg_mixer_stages(r[1], st, n_stages, c4 + 1);
    v.z = jg_mixer_stages(r[2], st, n_stages, c4 + 2);
    v.w = jg_mixer_stages(r[3], st, n_stages, c4 + 3);
    *reinterpret_cast<float4 *>(at(t) + c4) = v;
  }
}

// ---- the attention ops -------------------------------------------------------------------------------------------------
// The packed weights of an attention op (program.py: pack_frame_attn, pack_local_attn, pack_length_attn - one layout).
// The host folds the layer norms' gamma / beta into the kernels and biases that follow them and 1 / sqrt(D) into the
// query, in float64.  The feed-forward part is absent at F = 0 (frame attention alone allows that).
struct JgAttnWeights {
  const float *wqkv;       // [3][C][C]   (q | k | v, input channel, h D + d)
  const float *bqkv;       // [3][C]
  const float *wo;         // [C][C]      (h D + d, output channel)
  const float *bo;         // [C]
  const float *w1;         // [C][F]
  const float *b1;         // [F]
  const float *w2;         // [F][C]
  const float *b2;         // [C]
};
__device__ __forceinline__ JgAttnWeights jg_attn_weights(const float *w, int C, int F) {
  JgAttnWeights v;
  v.wqkv = w;
  v.bqkv = v.wqkv + 3 * C * C;
  v.wo = v.bqkv + 3 * C;
  v.bo = v.wo + C * C;
  v.w1 = v.bo + C;
  v.b1 = v.w1 + C * F;
  v.w2 = v.b1 + F;
  v.b2 = v.w2 + F * C;
  return v;
}

// x = x + Dense(C)(gelu(Dense(F)(LayerNormalization(x)))) on the residual registers of a wave's NBLK token blocks, 16
// hidden columns at a time.  The wave's rows go to xw, the workgroup's NTHREADS threads normalise the `ln_rows` rows of
// xn (xw lies inside them), the hidden columns pass through hid (NBLK x 16 rows of pitch 18).  Every thread of the
// workgroup calls this: the barriers are the workgroup's.
template <int C, int NBLK, int NTHREADS>
__device__ __forceinline__ void jg_attn_ffn(f32x4 (&xr)[NBLK][C / 16], float *xn, int ln_rows, float *xw, float *hid,
                                            const JgAttnWeights &w, int F, float eps, int tid, int n, int j) {
  constexpr int NB = C / 16, SX = C + 2, SH = 18;
  jg_mixer_put<C, NBLK>(xw, xr, n, j);
  __syncthreads();
  jg_mixer_layernorm<C, NTHREADS>(xn, ln_rows, tid, eps);
  jg_mixer_add_bias<C, NBLK>(xr, w.b2, n);
  __syncthreads();
  for (int hb = 0; hb < F; hb += 16) {
    f32x4 acc[NBLK];
    const float bias = w.b1[hb + n];
#pragma unroll
    for (int f = 0; f < NBLK; ++f) acc[f] = f32x4{bias, bias, bias, bias};
    jg_mixer_dense<NBLK, C>(xw, SX, w.w1 + hb + n, F, acc, n, j);
#pragma unroll
    for (int f = 0; f < NBLK; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) hid[(f * 16 + 4 * j + i) * SH + n] = jg_apply_act(acc[f][i], JG_ACT_GELU_TANH);
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float *__restrict__ w2col = w.w2 + (size_t)hb * C + nb * 16 + n;
#pragma unroll
      for (int k0 = 0; k0 < 16; k0 += 4) {
        const float b = w2col[(k0 + j) * C];
#pragma unroll
        for (int f = 0; f < NBLK; ++f)
          xr[f][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(hid[(f * 16 + n) * SH + k0 + j], b, xr[f][nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

// ---- host side of the attention ops ------------------------------------------------------------------------------------
// sizes the attention kernels cover (why: the reason when not): channels 32 and 64, and 16 with c16; key_dim = C / H;
// the feed-forward width, 0 with allow_F0 alone
static inline bool jg_attn_supports(bool c16, bool allow_F0, int C, int H, int F, char *why, size_t cap) {
  if (!(c16 && C == 16) && C != 32 && C != 64) {
    snprintf(why, cap, "%d channels (the kernel covers %s32 and 64)", C, c16 ? "16, " : "");
    return false;
  }
  const int D = H >= 1 && C % H == 0 ? C / H : 0;
  if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) {
    snprintf(why, cap, "%d heads at %d channels (key_dim = channels / heads must be 4, 8, 16, 32 or 64)", H, C);
    return false;
  }
  if (!(allow_F0 && F == 0) && (F % 16 != 0 || F < 16 || F > 256)) {
    snprintf(why, cap, "feed-forward width %d (%sa multiple of 16 up to 256)", F, allow_F0 ? "0, or " : "");
    return false;
  }
  return true;
}

// floats of the packed weights (JgAttnWeights)
static inline int64_t jg_attn_blob_floats(int C, int F) {
  return (int64_t)4 * C * C + 4 * C + (F > 0 ? (int64_t)2 * C * F + F + C : 0);
}

// launch of one kernel instantiation with `lds` bytes of dynamic LDS; `opened` is that instantiation's own: the largest
// size it was opened for so far
template <typename Args>
static inline int jg_mixer_launch(void (*kern)(Args), int64_t &opened, int64_t grid, int threads, int64_t lds, hipStream_t s, const Args &a) {
  if (lds > opened) {
    JG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    opened = lds;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), (size_t)lds, s, a);
  JG_HIP(hipGetLastError());
  return JG_OK;
}
