// One MaskedBiLSTM (reference: nnlib/v2/layers.py:1335-1430 - Keras 3 Bidirectional(LSTM(U, return_sequences=True),
// merge_mode="concat") on the frame rows, LSTMCell at its defaults).  Per direction, from h = c = 0, at step t:
//   z = x_t W + h R + b                       W (C, 4U), R (U, 4U), b (4U); the four U-wide slices of z are i, f, g, o
//   c' = sigmoid(f) c + sigmoid(i) tanh(g);   h' = sigmoid(o) tanh(c');   the step writes h'
// and under a mask (backend.rnn, zero_output_for_mask False) a masked step keeps c and h and writes the direction's
// previous output - which is the kept h, zeros while no valid step has come.  The backward direction walks t = L - 1 .. 0,
// its outputs stand at their own positions in channels [U, 2U).
//
// The serial chain is L steps of h (rows, U) @ R (U, 4U); the parallelism is across rows and the two directions.  A
// workgroup owns JG_BILSTM_ROWS = 16 rows (row = window * frames + frame, across the windows of the launch group; the last
// group is ragged) of ONE direction - the M block of v_mfma_f32_16x16x4_f32.  The host permutes the 4U gate columns so
// that wave w owns units 16 w .. 16 w + 15 of all four gates (U / 16 waves): lane (n, j) then holds i, f, g, o of unit
// 16 w + n and rows 4 j .. 4 j + 3 in its own accumulators, and the c / h update, the per-row mask select and the carried
// output are register work with no cross-lane traffic.
//   * R: the wave's slice stays in registers for the whole row (U / 4 x 4 floats a lane: 64 at U = 64).
//   * h: through a double-buffered LDS tile at the C + 2 pitch of jg_mixer_dev.h, one barrier a step.
//   * x_t W + b has no dependence on h: it is formed JG_BILSTM_STEPS = 8 steps ahead, in the same accumulator layout, and
//     kept in registers (8 x 16 a lane); the 16 rows x 8 steps of x go through LDS as the A operand, one float4 of W's
//     permuted row per lane and k serves the 32 products of the 8 steps.  A step's accumulators start from it: one
//     k-ordered fmaf chain from the bias over C inputs, then over U state values.
//   * a masked position's x is never loaded (a zero row in LDS) and its step's results are dropped by a select.
// LDS: 2 x 16 x (U + 2) + 8 x 16 x (C + 2) floats + 128 validity words: 74 KB at U = 64, C = 128, 22 KB at the fixture's
// 32 / 32.  Rows never touch each other: every index is row * L + position with row < rows and position < L.
#include "jg_common.h"
#include "jg_bilstm.h"
#include "jg_mixer_dev.h"

namespace {

constexpr int RB = JG_BILSTM_ROWS, S = JG_BILSTM_STEPS;
static_assert(RB == 16, "one 16-row block of the matrix cores");

// sigmoid and tanh through v_exp_f32 / v_rcp_f32 (jg_apply_act's sigmoid): absolute errors of about 1e-7, which is what the
// state update sees (tests/test_gpu_bilstm.py holds every op inside the bound its float32 emulation sets); 2^t -> 0 or inf
// saturates to the exact limits
__device__ __forceinline__ float lstm_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950f * v)); }
__device__ __forceinline__ float lstm_tanh(float v) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.8853900f * v)) - 1.0f; }

template <int U>
__global__ __launch_bounds__(U * 4) void bilstm_kernel(JgBilstmArgs a) {
  constexpr int NT = U * 4, SH = U + 2, KR = U / 4, G4 = 4 * U;
  extern __shared__ float lds[];
  const int C = a.C, SX = C + 2, C4 = C / 4, L = a.L;
  float *hl = lds;                                        // [2][16][SH]
  float *xl = hl + 2 * RB * SH;                           // [S][16][SX]
  int *vl = reinterpret_cast<int *>(xl + S * RB * SX);    // [S][16]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, j = lane >> 4;
  const int dir = blockIdx.x & 1, row0 = (blockIdx.x >> 1) * RB;
  const float *__restrict__ wp = a.w + (size_t)dir * ((size_t)(C + U + 1) * G4);      // W [C][4U]
  const float *__restrict__ rp = wp + (size_t)C * G4;                                 // R [U][4U]
  const float *__restrict__ bp = rp + (size_t)U * G4;                                 // b [4U]
  const int col4 = (wv * 16 + n) * 4, unit = wv * 16 + n, ch = dir * U + unit;
  f32x4 R[KR];
#pragma unroll
  for (int kk = 0; kk < KR; ++kk) R[kk] = *reinterpret_cast<const f32x4 *>(rp + (size_t)(4 * kk + j) * G4 + col4);
  const f32x4 bias = *reinterpret_cast<const f32x4 *>(bp + col4);
  for (int q = tid; q < RB * SH; q += NT) hl[q] = 0.f;
  float c[4] = {0.f, 0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f};
  int cur = 0;
  for (int q0 = 0; q0 < L; q0 += S) {
    __syncthreads();
    // the block's 16 rows x S steps of x (token s 16 + r: step q0 + s of row row0 + r), zero rows where there is none
    for (int q = tid; q < S * RB * C4; q += NT) {
      const int tok = q / C4, c4 = (q - tok * C4) * 4, step = q0 + (tok >> 4), row = row0 + (tok & 15);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (step < L && row < a.rows) {
        const size_t at = (size_t)row * L + (dir ? L - 1 - step : step);
        if (a.mask == nullptr || a.mask[at] != 0) v = *reinterpret_cast<const float4 *>(a.x + at * C + c4);
      }
      float *r = xl + tok * SX + c4;
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    }
    for (int q = tid; q < S * RB; q += NT) {
      const int step = q0 + (q >> 4), row = row0 + (q & 15);
      int ok = 0;
      if (step < L && row < a.rows) ok = a.mask == nullptr || a.mask[(size_t)row * L + (dir ? L - 1 - step : step)] != 0;
      vl[q] = ok;
    }
    __syncthreads();
    f32x4 pre[S][4];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[s][g] = f32x4{bias[g], bias[g], bias[g], bias[g]};
    for (int k0 = 0; k0 < C; k0 += 4) {
      const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wp + (size_t)(k0 + j) * G4 + col4);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const float xa = xl[(s * RB + n) * SX + k0 + j];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[s][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, w4[g], pre[s][g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (q0 + s < L) {                                   // (the same for the whole workgroup)
        const float *hc = hl + cur * RB * SH;
        float *hn = hl + (cur ^ 1) * RB * SH;
        f32x4 acc[4] = {pre[s][0], pre[s][1], pre[s][2], pre[s][3]};
#pragma unroll
        for (int kk = 0; kk < KR; ++kk) {
          const float ha = hc[n * SH + 4 * kk + j];
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha, R[kk][g], acc[g], 0, 0, 0);
        }
        const int t = dir ? L - 1 - (q0 + s) : q0 + s;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * j + i, row = row0 + r;
          const float ig = lstm_sigmoid(acc[0][i]), fg = lstm_sigmoid(acc[1][i]), gg = lstm_tanh(acc[2][i]), og = lstm_sigmoid(acc[3][i]);
          const float cn = fmaf(fg, c[i], ig * gg);
          const float hv = og * lstm_tanh(cn);
          const bool ok = vl[s * RB + r] != 0;
          c[i] = ok ? cn : c[i];
          h[i] = ok ? hv : h[i];
          hn[r * SH + unit] = h[i];
          if (row < a.rows) a.y[((size_t)row * L + t) * (2 * U) + ch] = jg_mixer_stages(h[i], a.st, a.n_stages, ch);
        }
        __syncthreads();
        cur ^= 1;
      }
    }
  }
}

template <int U>
int launch_u(const JgBilstmArgs &a, int64_t lds, hipStream_t s) {
  static int64_t opened = 0;
  const int64_t groups = ((int64_t)a.rows + RB - 1) / RB;
  return jg_mixer_launch(bilstm_kernel<U>, opened, 2 * groups, U * 4, lds, s, a);
}

}  // namespace

bool jg_bilstm_supports(int C, int U, int cout, char *why, size_t cap) {
  if (U != 16 && U != 32 && U != 64) {
    snprintf(why, cap, "%d units (the kernel covers 16, 32 and 64)", U);
    return false;
  }
  if (cout != 2 * U) {
    snprintf(why, cap, "%d output channels (the two directions side by side: 2 x %d units = %d)", cout, U, 2 * U);
    return false;
  }
  if (C < 16 || C > JG_BILSTM_MAX_C || C % 16 != 0) {
    snprintf(why, cap, "%d incoming channels (a multiple of 16 up to %d)", C, JG_BILSTM_MAX_C);
    return false;
  }
  return true;
}

int64_t jg_bilstm_blob_floats(int C, int U) { return (int64_t)2 * (C + U + 1) * 4 * U; }

int64_t jg_bilstm_lds_bytes(int C, int U) {
  return ((int64_t)2 * RB * (U + 2) + (int64_t)S * RB * (C + 2) + (int64_t)S * RB) * (int64_t)sizeof(float);
}

int jg_launch_bilstm(jg_engine *e, const JgBilstmArgs &a, hipStream_t s) {
  (void)e;
  char why[160];
  JG_REQUIRE(jg_bilstm_supports(a.C, a.U, 2 * a.U, why, sizeof(why)), JG_ERR_UNSUPPORTED, "bilstm: %s", why);
  JG_REQUIRE(a.x != nullptr && a.y != nullptr && a.w != nullptr && a.rows >= 1 && a.L >= 1 && (int64_t)a.rows / RB + 1 <= 0x3fffffff,
             JG_ERR_INVALID, "bilstm: bad launch arguments");
  JG_REQUIRE(a.y != a.x, JG_ERR_INVALID, "bilstm: the op cannot run in place");
  const int64_t lds = jg_bilstm_lds_bytes(a.C, a.U);
  JG_REQUIRE(lds <= 160 * 1024, JG_ERR_UNSUPPORTED, "bilstm: %lld bytes of LDS", (long long)lds);
  return a.U == 16 ? launch_u<16>(a, lds, s) : a.U == 32 ? launch_u<32>(a, lds, s) : launch_u<64>(a, lds, s);
}
