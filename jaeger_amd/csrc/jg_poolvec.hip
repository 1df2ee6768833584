// JG_OP_POOLVEC: one masked global pool over the (frames, length) rows of a window, merged into a range of a vector slot.
// The pooled branches of the reference's parallel_branches (nnlib/builder.py:1109-1153: every branch its own pooling, the
// vectors concatenated, summed, averaged or maximised in branch order) and MaskedLastPooling (nnlib/v2/layers.py:541-578).
//
// One workgroup per window.  MAX and AVG sweep the window as pool_kernel does (jg_kernels.hip: 256 / (c / 4) position groups of
// c / 4 threads, one float4 each, the groups folded through LDS in group order - the same sums in the same order); LAST counts
// every frame's mask bytes with a wave reduction and reads `frames` rows only.  The merge is a read-modify-write of the slot by
// the lane that owns the channel: the ops of one model are stream-ordered and a window's range belongs to one workgroup, so no
// atomics, and the branch order fixes the float32 result.
#include "jg_poolvec.h"

namespace {

__device__ __forceinline__ float merge_one(float prev, float r, int merge, float scale) {
  const float v = merge == JG_POOLVEC_ADD ? prev + r : merge == JG_POOLVEC_MAX ? fmaxf(prev, r) : r;
  return v * scale;
}

__global__ __launch_bounds__(256) void poolvec_sweep_kernel(JgPoolVecArgs a) {
  __shared__ float4 red[256];
  __shared__ float redc[256];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int c = a.c, positions = a.frames * a.L;
  const int cq = c >> 2;
  const int groups = 256 / cq;
  const int q = tid % cq, g = tid / cq;
  const bool is_max = a.kind != JG_POOL_AVG;
  float4 acc = is_max ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0.f, 0.f, 0.f, 0.f);
  float cnt = 0.f;
  if (g < groups) {
    const float *xb = a.x + (size_t)w * positions * c + q * 4;
    const uint8_t *mb = a.mask != nullptr ? a.mask + (size_t)w * positions : nullptr;
    for (int p = g; p < positions; p += groups) {
      const bool keep = mb == nullptr || mb[p] != 0;
      if (!keep) continue;
      const float4 v = *reinterpret_cast<const float4 *>(xb + (size_t)p * c);
      cnt += 1.f;
      if (is_max) {
        acc.x = fmaxf(acc.x, v.x); acc.y = fmaxf(acc.y, v.y);
        acc.z = fmaxf(acc.z, v.z); acc.w = fmaxf(acc.w, v.w);
      } else {
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
  }
  red[tid] = acc;
  redc[tid] = cnt;
  __syncthreads();
  if (g != 0) return;
  for (int gg = 1; gg < groups; ++gg) {
    const float4 t = red[gg * cq + q];
    cnt += redc[gg * cq + q];
    if (is_max) {
      acc.x = fmaxf(acc.x, t.x); acc.y = fmaxf(acc.y, t.y);
      acc.z = fmaxf(acc.z, t.z); acc.w = fmaxf(acc.w, t.w);
    } else {
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
  }
  float4 r;
  if (is_max) {
    // layers.py:517-529: masked positions lose to the -1e9 sentinel; a window with no valid position pools to zeros.
    // Without a mask: plain max
    if (a.mask == nullptr) {
      r = acc;
    } else if (cnt <= 0.f) {
      r = make_float4(0.f, 0.f, 0.f, 0.f);
    } else if (cnt < (float)positions) {
      r = make_float4(fmaxf(acc.x, -1.0e9f), fmaxf(acc.y, -1.0e9f), fmaxf(acc.z, -1.0e9f), fmaxf(acc.w, -1.0e9f));
    } else {
      r = acc;
    }
  } else {
    // layers.py:460-480: sum(x * m) / max(sum(m), 1e-7); plain mean without a mask
    const float d = a.mask != nullptr ? fmaxf(cnt, 1e-7f) : (float)positions;
    r = make_float4(acc.x / d, acc.y / d, acc.z / d, acc.w / d);
  }
  float4 *dst = reinterpret_cast<float4 *>(a.out + (size_t)w * a.out_ld + q * 4);
  float4 prev = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.merge != JG_POOLVEC_STORE) prev = *dst;
  *dst = make_float4(merge_one(prev.x, r.x, a.merge, a.scale), merge_one(prev.y, r.y, a.merge, a.scale),
                     merge_one(prev.z, r.z, a.merge, a.scale), merge_one(prev.w, r.w, a.merge, a.scale));
}

// MaskedLastPooling.call (layers.py:556-569), the code and not its docstring: idx = (valid positions of the frame row) - 1 -
// the COUNT, not the index of the last valid position; the row's value at max(idx, 0) is read whatever its mask byte says;
// frames with idx < 0 add zeros; the sum over the frames is divided by max(frames with idx >= 0, 1).  Without a mask: the
// mean over the frames of position L - 1
__global__ __launch_bounds__(256) void poolvec_last_kernel(JgPoolVecArgs a) {
  __shared__ int idx[JG_POOLVEC_MAX_FRAMES];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frames = a.frames, L = a.L, c = a.c;
  for (int f = wave; f < frames; f += 4) {
    int n = L;
    if (a.mask != nullptr) {
      const uint8_t *mb = a.mask + ((size_t)w * frames + f) * L;
      n = 0;
      for (int p = lane; p < L; p += 64) n += mb[p] != 0 ? 1 : 0;
      for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    }
    if (lane == 0) idx[f] = n - 1;
  }
  __syncthreads();
  int valid = 0;
  for (int f = 0; f < frames; ++f) valid += idx[f] >= 0 ? 1 : 0;
  const float div = a.mask != nullptr ? (float)max(valid, 1) : (float)frames;
  const float *xb = a.x + (size_t)w * frames * L * c;
  for (int ch = tid; ch < c; ch += 256) {
    float sum = 0.f;
    for (int f = 0; f < frames; ++f)
      if (idx[f] >= 0) sum += xb[((size_t)f * L + idx[f]) * c + ch];
    float *dst = a.out + (size_t)w * a.out_ld + ch;
    const float prev = a.merge != JG_POOLVEC_STORE ? *dst : 0.f;
    *dst = merge_one(prev, sum / div, a.merge, a.scale);
  }
}

}  // namespace

bool jg_poolvec_supports(int kind, int merge, int c, int vec_off, char *why, size_t cap) {
  if (kind != JG_POOL_MAX && kind != JG_POOL_AVG && kind != JG_POOL_LAST) {
    snprintf(why, cap, "pool kind %d (max %d, average %d or last %d)", kind, JG_POOL_MAX, JG_POOL_AVG, JG_POOL_LAST);
    return false;
  }
  if (merge != JG_POOLVEC_STORE && merge != JG_POOLVEC_ADD && merge != JG_POOLVEC_MAX) {
    snprintf(why, cap, "merge code %d (store %d, add %d or max %d)", merge, JG_POOLVEC_STORE, JG_POOLVEC_ADD, JG_POOLVEC_MAX);
    return false;
  }
  if (c < 4 || c % 4 != 0 || vec_off < 0 || vec_off % 4 != 0) {
    snprintf(why, cap, "%d channels at offset %d (both a multiple of 4: a lane owns four floats)", c, vec_off);
    return false;
  }
  if ((int64_t)vec_off + c > JG_POOLVEC_MAX_WIDTH) {
    snprintf(why, cap, "offset %d + %d channels beyond the vector slot's %d floats", vec_off, c, JG_POOLVEC_MAX_WIDTH);
    return false;
  }
  return true;
}

int jg_launch_poolvec(const JgPoolVecArgs &a, hipStream_t s) {
  char why[160];
  JG_REQUIRE(jg_poolvec_supports(a.kind, a.merge, a.c, 0, why, sizeof(why)), JG_ERR_UNSUPPORTED, "poolvec: %s", why);
  JG_REQUIRE(a.x != nullptr && a.out != nullptr && a.out_ld % 4 == 0 && a.out_ld >= a.c && a.frames >= 1 && a.L >= 1 &&
                 a.frames <= JG_POOLVEC_MAX_FRAMES,
             JG_ERR_INVALID, "poolvec: bad geometry (%d frames of %d positions, %d channels into rows of %d)", a.frames, a.L, a.c, a.out_ld);
  if (a.n_win == 0) return JG_OK;
  if (a.kind == JG_POOL_LAST) hipLaunchKernelGGL(poolvec_last_kernel, dim3((unsigned)a.n_win), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(poolvec_sweep_kernel, dim3((unsigned)a.n_win), dim3(256), 0, s, a);
  JG_HIP(hipGetLastError());
  return JG_OK;
}
