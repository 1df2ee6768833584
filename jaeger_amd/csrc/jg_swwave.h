// Smith-Waterman systolic wavefront, the device core of termini_kernel (jg_termini.hip) and align_kernel<R, T, REF>
// (jg_alignpairs.hip): local alignment of an n-row query against an m-column reference, match +2 / mismatch -100, a gap
// of k costs 100 + 5(k-1); letters compare case-insensitively and only A/C/G/T match (parasail.matrix_create("ACGT", 2,
// -100)).  No traceback matrix: every state carries counts of its best path (a count policy, below), and the counts of the
// best cell are the answer.
//
// One workgroup of T threads per job (T: a template parameter of everything below that depends on it - termini_kernel runs
// 256, align_kernel 256 or 512).  Thread t owns the query rows [t R, (t + 1) R) and walks its strip column by column
// one step behind thread t - 1: the only values that cross threads are the H / F states of each strip's last row,
// double-buffered in LDS, one barrier per step; threads without rows stay idle, m + n_active - 1 steps.
// Ties - the contract with parasail's traceback, written once here: H prefers the diagonal, then the gap in the query row
// (E), then F; E and F prefer extension; the best cell is the first maximum in (column, row) order.  parasail is not
// installable here: parity with its tie-breaking is unpinned (scores are unique; counts can differ only between co-optimal
// alignments).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int NEG = -1000000;       // "minus infinity" that survives a few subtractions
constexpr int S_MATCH = 2, S_MISMATCH = -100, G_OPEN = 100, G_EXT = 5;

__device__ __forceinline__ int base_code(uint8_t c) {   // A,C,G,T -> 0..3 (any case), else 4
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}

// ref[j], j < m, = the code of bases[r_off + j], or with rev that of complement(bases[r_off + m - 1 - j]); the caller's next
// barrier publishes it (sw_wavefront has one in front of its first step)
template <int T>
__device__ __forceinline__ void sw_load_ref(uint8_t *ref, const uint8_t *__restrict__ bases, int64_t r_off, int m, bool rev) {
  for (int j = threadIdx.x; j < m; j += T) {
    int c = rev ? base_code(bases[r_off + m - 1 - j]) : base_code(bases[r_off + j]);
    if (rev && c < 4) c = 3 - c;                                     // A<->T, C<->G on ACGT = 0..3
    ref[j] = (uint8_t)c;
  }
}

// ---- count policies: what a state's best path carries besides its score ---------------------------------------------
// A strip edge is the (H, H counts, F, F counts) of a strip's last row at one column: EDGE_PLANES int4 per thread and
// buffer, plane p of slot s at edge[p * 2 * T + s].

// columns << 16 | gaps in the query row (the largest is 2 * 4 096)
struct Counts2 {
  int a;
  static constexpr int EDGE_PLANES = 1;
  static __device__ __forceinline__ Counts2 zero() { return {0}; }
  __device__ __forceinline__ Counts2 query_gap() const { return {a + ((1 << 16) | 1)}; }   // one more column + query-row gap
  __device__ __forceinline__ Counts2 ref_gap() const { return {a + (1 << 16)}; }           // one more column + reference-row gap
  __device__ __forceinline__ Counts2 diagonal(bool) const { return {a + (1 << 16)}; }
  template <int T>
  static __device__ __forceinline__ void put(int4 *edge, int slot, int h, Counts2 hc, int f, Counts2 fc) {
    edge[slot] = make_int4(h, hc.a, f, fc.a);
  }
  template <int T>
  static __device__ __forceinline__ void get(const int4 *edge, int slot, int &h, Counts2 &hc, int &f, Counts2 &fc) {
    const int4 e = edge[slot];
    h = e.x; hc.a = e.y; f = e.z; fc.a = e.w;
  }
};

// four 16-bit fields of two ints (the largest is q_len + r_len = 24 576, columns of a 12 288 x 12 288 job; a0 stays below
// 2^31): a0 = columns << 16 | gaps in the query row,
// a1 = gaps in the reference row << 16 | identical columns
struct alignas(8) Counts4 {
  int a0, a1;
  static constexpr int EDGE_PLANES = 2;   // (H, Ha0, Ha1, pad) and (F, Fa0, Fa1, pad)
  static __device__ __forceinline__ Counts4 zero() { return {0, 0}; }
  __device__ __forceinline__ Counts4 query_gap() const { return {a0 + ((1 << 16) | 1), a1}; }
  __device__ __forceinline__ Counts4 ref_gap() const { return {a0 + (1 << 16), a1 + (1 << 16)}; }
  __device__ __forceinline__ Counts4 diagonal(bool same) const { return {a0 + (1 << 16), a1 + (same ? 1 : 0)}; }
  template <int T>
  static __device__ __forceinline__ void put(int4 *edge, int slot, int h, Counts4 hc, int f, Counts4 fc) {
    edge[slot] = make_int4(h, hc.a0, hc.a1, 0);
    edge[2 * T + slot] = make_int4(f, fc.a0, fc.a1, 0);
  }
  template <int T>
  static __device__ __forceinline__ void get(const int4 *edge, int slot, int &h, Counts4 &hc, int &f, Counts4 &fc) {
    const int4 eh = edge[slot], ef = edge[2 * T + slot];
    h = eh.x; hc.a0 = eh.y; hc.a1 = eh.z;
    f = ef.x; fc.a0 = ef.y; fc.a1 = ef.z;
  }
};

template <class Counts>
struct SwBest {      // a best cell: score 0 = none (counts zero, i = j = -1)
  int score;
  Counts counts;
  int i, j;          // row in the query, column in the reference
};

// ---- the wavefront --------------------------------------------------------------------------------------------------------
// The thread's best cell of the n x m job query = bases[q_off ..], ref = the m codes sw_load_ref wrote; R <= RMAX rows
// per thread, T * R >= n; edge: EDGE_PLANES * 2 * T int4 of LDS.  Ends behind a barrier.
template <int T, int RMAX, class Counts>
__device__ __forceinline__ SwBest<Counts> sw_wavefront(const uint8_t *__restrict__ bases, int64_t q_off, int n, int m, int R,
                                                       const uint8_t *ref, int4 *edge) {
  const int tid = threadIdx.x;
  const int i0 = tid * R;
  int q[RMAX], hl[RMAX], el[RMAX];
  Counts hlc[RMAX], elc[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    const int i = i0 + r;
    q[r] = (r < R && i < n) ? base_code(bases[q_off + i]) : 5;       // 5: row does not exist
    hl[r] = 0; hlc[r] = Counts::zero(); el[r] = NEG; elc[r] = Counts::zero();
  }
  Counts::template put<T>(edge, tid, 0, Counts::zero(), NEG, Counts::zero());
  Counts::template put<T>(edge, T + tid, 0, Counts::zero(), NEG, Counts::zero());
  SwBest<Counts> best{0, Counts::zero(), -1, -1};
  int prev_up_h = 0;                                                 // H[i0-1][j-1]
  Counts prev_up_c = Counts::zero();
  __syncthreads();
  const int n_active = (n + R - 1) / R;                              // threads that own rows (<= T)
  const int steps = m + n_active - 1;
  for (int step = 0; step < steps; ++step) {
    const int j = step - tid;
    int up_h = 0, up_f = NEG;
    Counts up_c = Counts::zero(), up_fc = Counts::zero();
    if (tid < n_active && j >= 0 && j < m) {
      if (tid > 0) Counts::template get<T>(edge, ((step + 1) & 1) * T + tid - 1, up_h, up_c, up_f, up_fc);   // written at step - 1
      int dg_h = prev_up_h;
      Counts dg_c = prev_up_c;
      prev_up_h = up_h; prev_up_c = up_c;
      const int rc = ref[j];
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        if (q[r] != 5) {
          // E: gap in the query row (consumes a ref base): from the left neighbour
          int e_s;
          Counts e_c;
          if (el[r] - G_EXT >= hl[r] - G_OPEN) { e_s = el[r] - G_EXT; e_c = elc[r]; }
          else { e_s = hl[r] - G_OPEN; e_c = hlc[r]; }
          e_c = e_c.query_gap();
          // F: gap in the ref row (consumes a query base): from above
          int f_s;
          Counts f_c;
          if (up_f - G_EXT >= up_h - G_OPEN) { f_s = up_f - G_EXT; f_c = up_fc; }
          else { f_s = up_h - G_OPEN; f_c = up_c; }
          f_c = f_c.ref_gap();
          const bool same = q[r] < 4 && q[r] == rc;
          int h = dg_h + (same ? S_MATCH : S_MISMATCH);
          Counts hc = dg_c.diagonal(same);
          if (e_s > h) { h = e_s; hc = e_c; }
          if (f_s > h) { h = f_s; hc = f_c; }
          if (h <= 0) { h = 0; hc = Counts::zero(); }
          if (h > best.score) { best.score = h; best.counts = hc; best.i = i0 + r; best.j = j; }
          dg_h = hl[r]; dg_c = hlc[r];                               // H[i][j-1] is the next row's diagonal
          hl[r] = h; hlc[r] = hc; el[r] = e_s; elc[r] = e_c;
          up_h = h; up_c = hc; up_f = f_s; up_fc = f_c;
        }
      }
    }
    Counts::template put<T>(edge, (step & 1) * T + tid, up_h, up_c, up_f, up_fc);
    __syncthreads();
  }
  return best;
}

// ---- the best cell of the job: max score, then smallest column, then smallest row --------------------------------------
// Tree reduction over the workgroup's SwBest (redk, redc: T entries of LDS each); the job's best cell, valid in thread 0.
// The key's 20-bit row and column fields hold the largest index of either wrapper, 12 287, with room to spare.
template <int T, class Counts>
__device__ __forceinline__ SwBest<Counts> sw_reduce_best(const SwBest<Counts> &mine, long long *redk, Counts *redc) {
  const int tid = threadIdx.x;
  redk[tid] = mine.score > 0 ? (((long long)mine.score << 40) | ((long long)(0xFFFFF - mine.j) << 20) | (long long)(0xFFFFF - mine.i)) : 0;
  redc[tid] = mine.counts;
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s && redk[tid + s] > redk[tid]) { redk[tid] = redk[tid + s]; redc[tid] = redc[tid + s]; }
    __syncthreads();
  }
  const long long k = redk[0];
  return {(int)(k >> 40), redc[0], k ? 0xFFFFF - (int)(k & 0xFFFFF) : -1, k ? 0xFFFFF - (int)((k >> 20) & 0xFFFFF) : -1};
}
