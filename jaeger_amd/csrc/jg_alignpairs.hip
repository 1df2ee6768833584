// Batched rectangular local alignment (the att-site search of postprocess/prophages.py:706-873): per prophage region the
// reference aligns the flank left of the region against the flank right of it with parasail's sw_trace_scan_16, direct and
// reverse-complemented, flanks of up to 4 000 + 2 000 bases.  Scoring and tie rules are termini_kernel's (jg_termini.hip):
// match +2 / mismatch -100, a gap of k costs 100 + 5(k-1), letters compare case-insensitively and only A/C/G/T match; H prefers
// the diagonal, then E (gap in the query row), then F; E and F prefer extension; the best cell is the first maximum in
// (column, row) order.
//
// align_kernel<R>: one workgroup per job, thread t owns the query rows [t R, (t + 1) R) and walks its strip column by column
// one step behind thread t - 1 (the systolic wavefront of termini_kernel): only the H / F states of each strip's last row
// cross threads, double-buffered in LDS, one barrier per step.  What differs from termini_kernel:
//   - the job is q_len x r_len (each 1 .. JG_ALIGN_MAX) and names its own spans; R is a template parameter chosen per job
//     (align_rows), threads without rows stay idle, r_len + n_active - 1 steps;
//   - every state's best path carries FOUR counts, packed as 16-bit fields of two ints (the largest is q_len + r_len =
//     12 288): a0 = columns << 16 | gaps in the query row, a1 = gaps in the reference row << 16 | identical columns.
// No traceback matrix is stored: the report's aligned strings are rebuilt on the host inside the (small) box the counts name.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jg_common.h"

namespace {

constexpr int AT = 256;          // threads per job
constexpr int ALIGN_MAX = JG_ALIGN_MAX;
constexpr int NEG = -1000000;    // "minus infinity" that survives a few subtractions
constexpr int S_MATCH = 2, S_MISMATCH = -100, G_OPEN = 100, G_EXT = 5;
constexpr int N_CLS = 6;
constexpr int ROW_CLS[N_CLS] = {1, 2, 4, 8, 16, 24};   // rows per thread of the instantiations: 256 R >= q_len

struct AlignJob {      // jg_align_job
  int64_t q_off;       // query[i] = bases[q_off + i]
  int64_t r_off;       // ref[j] = bases[r_off + j], or with flags & 1 complement(bases[r_off + r_len - 1 - j])
  int32_t q_len, r_len;
  int32_t flags;
  int32_t pad_;
};

struct AlignOut {
  int32_t score, cols, fgaps, rgaps, idents, end_q, end_r, zero;
};

// rows per thread a job of q_len query rows runs with: the smallest instantiation that covers it
inline int align_rows(int q_len) {
  for (int k = 0; k < N_CLS; ++k)
    if (ROW_CLS[k] * AT >= q_len) return ROW_CLS[k];
  return ROW_CLS[N_CLS - 1];
}

__device__ __forceinline__ int align_code(uint8_t c) {   // A,C,G,T -> 0..3 (any case), else 4
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}

template <int R>
__global__ __launch_bounds__(AT) void align_kernel(const uint8_t *__restrict__ bases, const AlignJob *__restrict__ jobs,
                                                   AlignOut *__restrict__ out) {
  // LDS: reference codes (ALIGN_MAX), strip edges [2][AT] as (H, Ha0, Ha1, pad) and (F, Fa0, Fa1, pad), reduction scratch
  __shared__ __attribute__((aligned(16))) uint8_t ref[ALIGN_MAX];
  __shared__ int4 edge_h[2 * AT], edge_f[2 * AT];
  __shared__ long long redk[AT];
  __shared__ int2 reda[AT];
  const AlignJob job = jobs[blockIdx.x];
  const int n = job.q_len, m = job.r_len, tid = threadIdx.x;
  const bool rev = (job.flags & 1) != 0;
  for (int j = tid; j < m; j += AT) {
    int c = rev ? align_code(bases[job.r_off + m - 1 - j]) : align_code(bases[job.r_off + j]);
    if (rev && c < 4) c = 3 - c;                                     // A<->T, C<->G on ACGT = 0..3
    ref[j] = (uint8_t)c;
  }
  const int i0 = tid * R;
  int q[R], hl[R], el[R], hl0[R], hl1[R], el0[R], el1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = i0 + r;
    q[r] = i < n ? align_code(bases[job.q_off + i]) : 5;            // 5: row does not exist
    hl[r] = 0; hl0[r] = 0; hl1[r] = 0; el[r] = NEG; el0[r] = 0; el1[r] = 0;
  }
  edge_h[tid] = make_int4(0, 0, 0, 0);
  edge_h[AT + tid] = make_int4(0, 0, 0, 0);
  edge_f[tid] = make_int4(NEG, 0, 0, 0);
  edge_f[AT + tid] = make_int4(NEG, 0, 0, 0);
  int best = 0, best0 = 0, best1 = 0, best_i = -1, best_j = -1;
  int prev_h = 0, prev_0 = 0, prev_1 = 0;                            // H[i0-1][j-1]
  __syncthreads();
  const int n_active = (n + R - 1) / R;                              // threads that own rows (<= AT: 256 R >= n)
  const int steps = m + n_active - 1;
  for (int step = 0; step < steps; ++step) {
    const int j = step - tid;
    int4 pub_h = make_int4(0, 0, 0, 0), pub_f = make_int4(NEG, 0, 0, 0);
    if (tid < n_active && j >= 0 && j < m) {
      int up_h = 0, up_0 = 0, up_1 = 0, up_f = NEG, up_f0 = 0, up_f1 = 0;
      if (tid > 0) {
        const int4 eh = edge_h[((step + 1) & 1) * AT + tid - 1];     // written at step - 1
        const int4 ef = edge_f[((step + 1) & 1) * AT + tid - 1];
        up_h = eh.x; up_0 = eh.y; up_1 = eh.z;
        up_f = ef.x; up_f0 = ef.y; up_f1 = ef.z;
      }
      int dg_h = prev_h, dg_0 = prev_0, dg_1 = prev_1;
      prev_h = up_h; prev_0 = up_0; prev_1 = up_1;
      const int rc = ref[j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (q[r] != 5) {
          // E: gap in the query row (consumes a ref base): from the left neighbour
          int e_s, e_0, e_1;
          if (el[r] - G_EXT >= hl[r] - G_OPEN) { e_s = el[r] - G_EXT; e_0 = el0[r]; e_1 = el1[r]; }
          else { e_s = hl[r] - G_OPEN; e_0 = hl0[r]; e_1 = hl1[r]; }
          e_0 += (1 << 16) | 1;                                      // one more column, one more query-row gap
          // F: gap in the ref row (consumes a query base): from above
          int f_s, f_0, f_1;
          if (up_f - G_EXT >= up_h - G_OPEN) { f_s = up_f - G_EXT; f_0 = up_f0; f_1 = up_f1; }
          else { f_s = up_h - G_OPEN; f_0 = up_0; f_1 = up_1; }
          f_0 += 1 << 16;
          f_1 += 1 << 16;                                            // one more column, one more reference-row gap
          const bool same = q[r] < 4 && q[r] == rc;
          int h = dg_h + (same ? S_MATCH : S_MISMATCH), h0 = dg_0 + (1 << 16), h1 = dg_1 + (same ? 1 : 0);
          if (e_s > h) { h = e_s; h0 = e_0; h1 = e_1; }
          if (f_s > h) { h = f_s; h0 = f_0; h1 = f_1; }
          if (h <= 0) { h = 0; h0 = 0; h1 = 0; }
          if (h > best) { best = h; best0 = h0; best1 = h1; best_i = i0 + r; best_j = j; }
          dg_h = hl[r]; dg_0 = hl0[r]; dg_1 = hl1[r];                // H[i][j-1] is the next row's diagonal
          hl[r] = h; hl0[r] = h0; hl1[r] = h1; el[r] = e_s; el0[r] = e_0; el1[r] = e_1;
          up_h = h; up_0 = h0; up_1 = h1; up_f = f_s; up_f0 = f_0; up_f1 = f_1;
        }
      }
      pub_h = make_int4(up_h, up_0, up_1, 0);
      pub_f = make_int4(up_f, up_f0, up_f1, 0);
    }
    edge_h[(step & 1) * AT + tid] = pub_h;
    edge_f[(step & 1) * AT + tid] = pub_f;
    __syncthreads();
  }
  // best cell of the job: max score, then smallest column, then smallest row
  redk[tid] = best > 0 ? (((long long)best << 40) | ((long long)(0xFFFFF - best_j) << 20) | (long long)(0xFFFFF - best_i)) : 0;
  reda[tid] = make_int2(best0, best1);
  __syncthreads();
  for (int s = AT / 2; s > 0; s >>= 1) {
    if (tid < s && redk[tid + s] > redk[tid]) { redk[tid] = redk[tid + s]; reda[tid] = reda[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const long long k = redk[0];
    const int2 a = reda[0];
    AlignOut o;
    o.score = (int)(k >> 40);
    o.cols = k ? a.x >> 16 : 0;
    o.fgaps = k ? a.x & 0xffff : 0;
    o.rgaps = k ? a.y >> 16 : 0;
    o.idents = k ? a.y & 0xffff : 0;
    o.end_r = k ? 0xFFFFF - (int)((k >> 20) & 0xFFFFF) : -1;
    o.end_q = k ? 0xFFFFF - (int)(k & 0xFFFFF) : -1;
    o.zero = 0;
    out[blockIdx.x] = o;
  }
}

template <int R>
int launch_align(const uint8_t *d_bases, const AlignJob *d_jobs, AlignOut *d_out, int n, hipStream_t s) {
  hipLaunchKernelGGL(align_kernel<R>, dim3((unsigned)n), dim3(AT), 0, s, d_bases, d_jobs, d_out);
  JG_HIP(hipGetLastError());
  return JG_OK;
}

struct DevMem {          // stream-ordered device allocation released with its scope
  void *p = nullptr;
  hipStream_t st = nullptr;
  DevMem() = default;
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { if (p) (void)hipFreeAsync(p, st); }
  int alloc(size_t bytes, hipStream_t s) {
    st = s;
    JG_HIP(hipMallocAsync(&p, std::max<size_t>(bytes, 1), s));
    return JG_OK;
  }
};

}  // namespace

// results: (n_jobs, 8) int32 on the host: score, columns, query-row gaps, reference-row gaps, identities, end in the query,
// end in the reference, 0; a job that scores 0 has counts 0 and ends -1.
extern "C" int jg_align_pairs(jg_engine *e, const uint8_t *bases, int64_t n_bases, int bases_loc, const void *jobs_v,
                              int64_t n_jobs, int32_t *results) {
  JG_REQUIRE(e != nullptr && n_jobs >= 0, JG_ERR_INVALID, "jg_align_pairs: bad arguments");
  if (n_jobs == 0) return JG_OK;
  JG_REQUIRE(bases != nullptr && jobs_v != nullptr && results != nullptr && n_bases >= 0 &&
                 (bases_loc == JG_PTR_HOST || bases_loc == JG_PTR_DEVICE) && n_jobs <= (int64_t)1 << 24,
             JG_ERR_INVALID, "jg_align_pairs: bad arguments");
  const AlignJob *jobs = static_cast<const AlignJob *>(jobs_v);
  for (int64_t k = 0; k < n_jobs; ++k) {
    const AlignJob &j = jobs[k];
    JG_REQUIRE(j.q_len >= 1 && j.q_len <= ALIGN_MAX && j.r_len >= 1 && j.r_len <= ALIGN_MAX, JG_ERR_UNSUPPORTED,
               "jg_align_pairs: job %lld is %d x %d (each length 1 .. %d)", (long long)k, j.q_len, j.r_len, ALIGN_MAX);
    JG_REQUIRE(j.q_off >= 0 && j.q_off <= n_bases - j.q_len && j.r_off >= 0 && j.r_off <= n_bases - j.r_len, JG_ERR_INVALID,
               "jg_align_pairs: job %lld has a span outside the %lld bases", (long long)k, (long long)n_bases);
  }
  // jobs bucketed by row class, tallest first (workgroups are dispatched in index order); call order inside a bucket
  std::vector<AlignJob> sorted;
  std::vector<int64_t> owner;
  int first[N_CLS + 1];
  sorted.reserve((size_t)n_jobs);
  owner.reserve((size_t)n_jobs);
  for (int c = N_CLS - 1; c >= 0; --c) {
    first[N_CLS - 1 - c] = (int)sorted.size();
    for (int64_t k = 0; k < n_jobs; ++k)
      if (align_rows(jobs[k].q_len) == ROW_CLS[c]) { sorted.push_back(jobs[k]); owner.push_back(k); }
  }
  first[N_CLS] = (int)sorted.size();
  JG_HIP(hipSetDevice(e->dev));
  hipStream_t s = e->stream;
  const uint8_t *d_bases = bases;
  DevMem tmp_bases, d_jobs, d_out;
  int rc;
  if (bases_loc == JG_PTR_HOST) {
    if ((rc = tmp_bases.alloc((size_t)n_bases, s)) != JG_OK) return rc;
    JG_HIP(hipMemcpyAsync(tmp_bases.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, s));
    d_bases = static_cast<const uint8_t *>(tmp_bases.p);
  }
  if ((rc = d_jobs.alloc(sorted.size() * sizeof(AlignJob), s)) != JG_OK) return rc;
  if ((rc = d_out.alloc(sorted.size() * sizeof(AlignOut), s)) != JG_OK) return rc;
  JG_HIP(hipMemcpyAsync(d_jobs.p, sorted.data(), sorted.size() * sizeof(AlignJob), hipMemcpyHostToDevice, s));
  const AlignJob *dj = static_cast<const AlignJob *>(d_jobs.p);
  AlignOut *dout = static_cast<AlignOut *>(d_out.p);
  for (int b = 0; b < N_CLS; ++b) {
    const int a = first[b], n = first[b + 1] - first[b];
    if (n == 0) continue;
    switch (ROW_CLS[N_CLS - 1 - b]) {
      case 1: rc = launch_align<1>(d_bases, dj + a, dout + a, n, s); break;
      case 2: rc = launch_align<2>(d_bases, dj + a, dout + a, n, s); break;
      case 4: rc = launch_align<4>(d_bases, dj + a, dout + a, n, s); break;
      case 8: rc = launch_align<8>(d_bases, dj + a, dout + a, n, s); break;
      case 16: rc = launch_align<16>(d_bases, dj + a, dout + a, n, s); break;
      default: rc = launch_align<24>(d_bases, dj + a, dout + a, n, s); break;
    }
    if (rc != JG_OK) return rc;
  }
  std::vector<AlignOut> host(sorted.size());
  JG_HIP(hipMemcpyAsync(host.data(), d_out.p, host.size() * sizeof(AlignOut), hipMemcpyDeviceToHost, s));
  JG_HIP(hipStreamSynchronize(s));
  static_assert(sizeof(AlignOut) == 8 * sizeof(int32_t) && sizeof(AlignJob) == 32, "jg_align_pairs: record layout");
  for (size_t k = 0; k < host.size(); ++k) memcpy(results + owner[k] * 8, &host[k], sizeof(AlignOut));
  return JG_OK;
}
