// Batched rectangular local alignment (the att-site search of postprocess/prophages.py:706-873): per prophage region the
// reference aligns the flank left of the region against the flank right of it with parasail's sw_trace_scan_16, direct and
// reverse-complemented.  A flank is scan_length + off_set bases: scan_length = min(max(int(0.04 len), 400), 4000) outside the
// region and off_set inside it, off_set = region_len // 4 while region_len // 2 < 14 000 and 2 000 above - up to
// 4 000 + 6 999 = 10 999 bases.  Scoring, tie rules and the systolic wavefront are the core of jg_swwave.h, shared with
// termini_kernel (jg_termini.hip).
//
// align_kernel<R, T, REF>: one workgroup of T threads per job, a thin wrapper of that core.  What differs from termini_kernel:
//   - the job is q_len x r_len and names its own spans; R is a template parameter chosen per job (align_rows) and the core
//     runs with RMAX = R; LDS is static, REF reference codes;
//   - every state's best path carries FOUR counts (Counts4): columns, gaps in the query row, gaps in the reference row,
//     identical columns.
// Two geometries of the one template: T = 256 with REF = JG_ALIGN_MAX (256 x 24 = 6 144) for a job whose two lengths are both
// at most JG_ALIGN_MAX - every job jg_align_pairs accepts, so a row does not depend on the entry point it came through - and
// T = 512 with REF = JG_ALIGN_LONG_MAX (512 x 24 = 12 288) for every other job of jg_align_pairs_long.
// No traceback matrix is stored: the report's aligned strings are rebuilt on the host inside the (small) box the counts name.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jg_host.h"
#include "jg_swwave.h"

namespace {

constexpr int AT = 256, ALIGN_MAX = JG_ALIGN_MAX;                 // threads per job and longest span, short geometry
constexpr int AT_LONG = 512, ALIGN_LONG_MAX = JG_ALIGN_LONG_MAX;  // the same of the long geometry
constexpr int N_ROWS = 6;
constexpr int ROWS[N_ROWS] = {24, 16, 8, 4, 2, 1};   // rows per thread of the instantiations (T R >= q_len)
static_assert(AT * ROWS[0] == ALIGN_MAX && AT_LONG * ROWS[0] == ALIGN_LONG_MAX, "the tallest class covers the longest span");
// a job's kernel class, in launch order: the long geometry's rows | CLS_LONG, then the short geometry's rows
constexpr int CLS_LONG = 64;
constexpr int N_CLS = 2 * N_ROWS;
constexpr int CLS_ORDER[N_CLS] = {CLS_LONG | 24, CLS_LONG | 16, CLS_LONG | 8, CLS_LONG | 4, CLS_LONG | 2, CLS_LONG | 1,
                                  24, 16, 8, 4, 2, 1};

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

// rows per thread a job of q_len query rows runs with on `threads` threads: the smallest instantiation that covers it
inline int align_rows(int q_len, int threads) {
  for (int k = N_ROWS - 1; k > 0; --k)
    if (ROWS[k] * threads >= q_len) return ROWS[k];
  return ROWS[0];
}

// the kernel class of a job: both lengths within the short geometry's span -> the 256-thread instantiations
inline int align_class(const AlignJob &j) {
  if (j.q_len <= ALIGN_MAX && j.r_len <= ALIGN_MAX) return align_rows(j.q_len, AT);
  return CLS_LONG | align_rows(j.q_len, AT_LONG);
}

template <int R, int T, int REF>
__global__ __launch_bounds__(T) void align_kernel(const uint8_t *__restrict__ bases, const AlignJob *__restrict__ jobs,
                                                  AlignOut *__restrict__ out) {
  // LDS: reference codes (REF), strip edges [2][T] in two planes, reduction scratch
  __shared__ __attribute__((aligned(16))) uint8_t ref[REF];
  __shared__ int4 edge[Counts4::EDGE_PLANES * 2 * T];
  __shared__ long long redk[T];
  __shared__ Counts4 redc[T];
  const AlignJob job = jobs[blockIdx.x];
  sw_load_ref<T>(ref, bases, job.r_off, job.r_len, (job.flags & 1) != 0);
  const SwBest<Counts4> mine = sw_wavefront<T, R, Counts4>(bases, job.q_off, job.q_len, job.r_len, R, ref, edge);
  const SwBest<Counts4> b = sw_reduce_best<T>(mine, redk, redc);
  if (threadIdx.x == 0)
    out[blockIdx.x] = AlignOut{b.score, b.counts.a0 >> 16, b.counts.a0 & 0xffff, b.counts.a1 >> 16, b.counts.a1 & 0xffff, b.i, b.j, 0};
}

template <int R, int T, int REF>
int launch_align(const uint8_t *d_bases, const AlignJob *d_jobs, AlignOut *d_out, int n, hipStream_t s) {
  hipLaunchKernelGGL((align_kernel<R, T, REF>), dim3((unsigned)n), dim3(T), 0, s, d_bases, d_jobs, d_out);
  JG_HIP(hipGetLastError());
  return JG_OK;
}

// one launch of the geometry's instantiation with `rows` rows per thread
template <int T, int REF>
int launch_rows(int rows, const uint8_t *d_bases, const AlignJob *d_jobs, AlignOut *d_out, int n, hipStream_t s) {
  switch (rows) {
    case 1: return launch_align<1, T, REF>(d_bases, d_jobs, d_out, n, s);
    case 2: return launch_align<2, T, REF>(d_bases, d_jobs, d_out, n, s);
    case 4: return launch_align<4, T, REF>(d_bases, d_jobs, d_out, n, s);
    case 8: return launch_align<8, T, REF>(d_bases, d_jobs, d_out, n, s);
    case 16: return launch_align<16, T, REF>(d_bases, d_jobs, d_out, n, s);
    default: return launch_align<24, T, REF>(d_bases, d_jobs, d_out, n, s);
  }
}

// jg_align_pairs (limit = JG_ALIGN_MAX) and jg_align_pairs_long (limit = JG_ALIGN_LONG_MAX): `name` is the entry point's,
// for the messages
int align_pairs_impl(jg_engine *e, const uint8_t *bases, int64_t n_bases, int bases_loc, const void *jobs_v, int64_t n_jobs,
                     int32_t *results, int limit, const char *name) {
  JG_REQUIRE(e != nullptr && n_jobs >= 0, JG_ERR_INVALID, "%s: bad arguments", name);
  if (n_jobs == 0) return JG_OK;
  JG_REQUIRE(bases != nullptr && jobs_v != nullptr && results != nullptr && n_bases >= 0 &&
                 (bases_loc == JG_PTR_HOST || bases_loc == JG_PTR_DEVICE) && n_jobs <= (int64_t)1 << 24,
             JG_ERR_INVALID, "%s: bad arguments", name);
  const AlignJob *jobs = static_cast<const AlignJob *>(jobs_v);
  for (int64_t k = 0; k < n_jobs; ++k) {
    const AlignJob &j = jobs[k];
    JG_REQUIRE(j.q_len >= 1 && j.q_len <= limit && j.r_len >= 1 && j.r_len <= limit, JG_ERR_UNSUPPORTED,
               "%s: job %lld is %d x %d (each length 1 .. %d)", name, (long long)k, j.q_len, j.r_len, limit);
    JG_REQUIRE(j.q_off >= 0 && j.q_off <= n_bases - j.q_len && j.r_off >= 0 && j.r_off <= n_bases - j.r_len, JG_ERR_INVALID,
               "%s: job %lld has a span outside the %lld bases", name, (long long)k, (long long)n_bases);
  }
  // jobs bucketed by kernel class, tallest first (workgroups are dispatched in index order); call order inside a bucket
  std::vector<AlignJob> sorted;
  std::vector<int64_t> owner;
  int first[N_CLS + 1];
  bucket_by_class(jobs, (size_t)n_jobs, CLS_ORDER, N_CLS, align_class, sorted, owner, first);
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
    const int cls = CLS_ORDER[b];
    rc = (cls & CLS_LONG) ? launch_rows<AT_LONG, ALIGN_LONG_MAX>(cls & ~CLS_LONG, d_bases, dj + a, dout + a, n, s)
                          : launch_rows<AT, ALIGN_MAX>(cls, d_bases, dj + a, dout + a, n, s);
    if (rc != JG_OK) return rc;
  }
  std::vector<AlignOut> host(sorted.size());
  if ((rc = download(host, d_out, s)) != JG_OK) return rc;
  static_assert(sizeof(AlignOut) == 8 * sizeof(int32_t) && sizeof(AlignJob) == 32, "jg_align_job / result row layout");
  for (size_t k = 0; k < host.size(); ++k) memcpy(results + owner[k] * 8, &host[k], sizeof(AlignOut));
  return JG_OK;
}

}  // namespace

// results: (n_jobs, 8) int32 on the host: score, columns, query-row gaps, reference-row gaps, identities, end in the query,
// end in the reference, 0; a job that scores 0 has counts 0 and ends -1.
extern "C" int jg_align_pairs(jg_engine *e, const uint8_t *bases, int64_t n_bases, int bases_loc, const void *jobs_v,
                              int64_t n_jobs, int32_t *results) {
  return align_pairs_impl(e, bases, n_bases, bases_loc, jobs_v, n_jobs, results, ALIGN_MAX, "jg_align_pairs");
}

// the same call for lengths of 1 .. JG_ALIGN_LONG_MAX
extern "C" int jg_align_pairs_long(jg_engine *e, const uint8_t *bases, int64_t n_bases, int bases_loc, const void *jobs_v,
                                   int64_t n_jobs, int32_t *results) {
  return align_pairs_impl(e, bases, n_bases, bases_loc, jobs_v, n_jobs, results, ALIGN_LONG_MAX, "jg_align_pairs_long");
}
