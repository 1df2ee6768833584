// Batched rectangular local alignment (the att-site search of postprocess/prophages.py:706-873): per prophage region the
// reference aligns the flank left of the region against the flank right of it with parasail's sw_trace_scan_16, direct and
// reverse-complemented, flanks of up to 4 000 + 2 000 bases.  Scoring, tie rules and the systolic wavefront are the core of
// jg_swwave.h, shared with termini_kernel (jg_termini.hip).
//
// align_kernel<R>: one workgroup per job, a thin wrapper of that core.  What differs from termini_kernel:
//   - the job is q_len x r_len (each 1 .. JG_ALIGN_MAX) and names its own spans; R is a template parameter chosen per job
//     (align_rows) and the core runs with RMAX = R; LDS is static;
//   - every state's best path carries FOUR counts (Counts4): columns, gaps in the query row, gaps in the reference row,
//     identical columns.
// No traceback matrix is stored: the report's aligned strings are rebuilt on the host inside the (small) box the counts name.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jg_host.h"
#include "jg_swwave.h"

namespace {

constexpr int AT = SW_T;         // threads per job
constexpr int ALIGN_MAX = JG_ALIGN_MAX;
constexpr int N_CLS = 6;
constexpr int ROW_CLS[N_CLS] = {24, 16, 8, 4, 2, 1};   // rows per thread of the instantiations (256 R >= q_len), in launch order

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
  for (int k = N_CLS - 1; k > 0; --k)
    if (ROW_CLS[k] * AT >= q_len) return ROW_CLS[k];
  return ROW_CLS[0];
}

template <int R>
__global__ __launch_bounds__(AT) void align_kernel(const uint8_t *__restrict__ bases, const AlignJob *__restrict__ jobs,
                                                   AlignOut *__restrict__ out) {
  // LDS: reference codes (ALIGN_MAX), strip edges [2][AT] in two planes, reduction scratch
  __shared__ __attribute__((aligned(16))) uint8_t ref[ALIGN_MAX];
  __shared__ int4 edge[Counts4::EDGE_PLANES * 2 * AT];
  __shared__ long long redk[AT];
  __shared__ Counts4 redc[AT];
  const AlignJob job = jobs[blockIdx.x];
  sw_load_ref(ref, bases, job.r_off, job.r_len, (job.flags & 1) != 0);
  const SwBest<Counts4> mine = sw_wavefront<R, Counts4>(bases, job.q_off, job.q_len, job.r_len, R, ref, edge);
  const SwBest<Counts4> b = sw_reduce_best(mine, redk, redc);
  if (threadIdx.x == 0)
    out[blockIdx.x] = AlignOut{b.score, b.counts.a0 >> 16, b.counts.a0 & 0xffff, b.counts.a1 >> 16, b.counts.a1 & 0xffff, b.i, b.j, 0};
}

template <int R>
int launch_align(const uint8_t *d_bases, const AlignJob *d_jobs, AlignOut *d_out, int n, hipStream_t s) {
  hipLaunchKernelGGL(align_kernel<R>, dim3((unsigned)n), dim3(AT), 0, s, d_bases, d_jobs, d_out);
  JG_HIP(hipGetLastError());
  return JG_OK;
}

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
  bucket_by_class(jobs, (size_t)n_jobs, ROW_CLS, N_CLS, [](const AlignJob &j) { return align_rows(j.q_len); }, sorted,
                  owner, first);
  JG_HIP(hipSetDevice(e->dev));
  hipStream_t s = e->stream;
  const uint8_t *d_bases = bases;
  DevBuf tmp_bases, d_jobs, d_out;
  int rc;
  if (bases_loc == JG_PTR_HOST) {
    if ((rc = tmp_bases.alloc((size_t)n_bases, s)) != JG_OK) return rc;
    JG_HIP(hipMemcpyAsync(tmp_bases.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, s));
    d_bases = tmp_bases.as<const uint8_t>();
  }
  if ((rc = upload(d_jobs, sorted, s)) != JG_OK) return rc;
  if ((rc = d_out.alloc(sorted.size() * sizeof(AlignOut), s)) != JG_OK) return rc;
  const AlignJob *dj = d_jobs.as<const AlignJob>();
  AlignOut *dout = d_out.as<AlignOut>();
  for (int b = 0; b < N_CLS; ++b) {
    const int a = first[b], n = first[b + 1] - first[b];
    if (n == 0) continue;
    switch (ROW_CLS[b]) {
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
  if ((rc = download(host, d_out, s)) != JG_OK) return rc;
  static_assert(sizeof(AlignOut) == 8 * sizeof(int32_t) && sizeof(AlignJob) == 32, "jg_align_pairs: record layout");
  for (size_t k = 0; k < host.size(); ++k) memcpy(results + owner[k] * 8, &host[k], sizeof(AlignOut));
  return JG_OK;
}
