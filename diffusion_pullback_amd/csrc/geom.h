// Device pieces shared by the geometry kernels (orth.hip, angles.hip, frechet.hip, flagmean.hip, geodesic.hip, transport.hip, hungarian.hip) and the chain
// kernels (chain.hip, hguide.hip): the round-robin Jacobi eigen-solve, the fixed-order block sum, the guarded four-column row access, rows cut into slices
// with fixed-order fp64 sums, the row-group step of the fp64 MFMA streams and the descending rank order.
#pragma once
#include "kernels.h"
#include "rank.h"      // sorts_before, rank_desc (one total order, NaN first, for every kernel that scatters by rank), max_nan

namespace dpb {

typedef double geom_d4 __attribute__((ext_vector_type(4)));

__device__ inline double nan64() { return __longlong_as_double(0x7ff8000000000000LL); }

// ------------------------------------------------------------------------------------------------------------ the eigen-solve
// A [k][k] symmetric in LDS -> diagonal; with eigenvectors, V <- V J for every rotation J (the caller starts it at the identity: A_in = V diag V^T).
// Two-sided Jacobi in the round-robin (tournament) order: a step rotates floor(k/2) DISJOINT index pairs at once -- the angle of a pair (p, q) depends on
// A[p][p], A[q][q], A[p][q] only, which no other pair of the step touches, so a step is the product of its rotations in any order: A <- A J for every row
// (and V <- V J), barrier, A <- J^T A for every column, barrier.  k - 1 (k even) or k steps make a sweep that visits every pair once.  Every thread of the
// workgroup of NT calls it, after a barrier that follows the last store to A and V; it returns after one.
template <int KMAX>
struct JacobiWs {
  double rc[KMAX / 2 + 1], rsn[KMAX / 2 + 1], red[2][16];
  int rp[KMAX / 2 + 1], rq[KMAX / 2 + 1];
};

// where the eigenvectors live: nowhere, in an LDS array, or transposed in global memory (the lanes of a wave walk the rows of V: coalesced)
struct JacobiNoVecs { static constexpr bool none = true; };
template <int KMAX>
struct JacobiLdsVecs {
  static constexpr bool none = false;
  double (*V)[KMAX + 1];
  __device__ __forceinline__ double& at(int i, int j) const { return V[i][j]; }
};
struct JacobiGlobalVecsT {
  static constexpr bool none = false;
  double* Vt; int k;
  __device__ __forceinline__ double& at(int i, int j) const { return Vt[(long)j * k + i]; }
};

template <int KMAX, int NT, typename Vecs>
__device__ __forceinline__ void jacobi_round_robin(double (*A)[KMAX + 1], Vecs V, JacobiWs<KMAX>& w, int k) {
  constexpr int NW = NT / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m = (k + 1) & ~1, half = m / 2, steps = m - 1;      // players 0 .. m-1 (player k is a bye when k is odd)
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0, diag = 0;                    // converged when the off-diagonal mass is negligible: fixed-order reduction, uniform result
    for (int r = wave; r < k; r += NW)
      for (int c = lane; c < k; c += 64) {
        const double v = A[r][c] * A[r][c];
        if (r == c) diag += v; else if (r < c) off += v;
      }
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); diag += __shfl_xor(diag, o, 64); }
    if (lane == 0) { w.red[0][wave] = off; w.red[1][wave] = diag; }
    __syncthreads();
    off = 0; diag = 0;
#pragma unroll
    for (int x = 0; x < NW; ++x) { off += w.red[0][x]; diag += w.red[1][x]; }
    __syncthreads();
    if (off <= 1e-28 * diag) break;
    for (int st = 0; st < steps; ++st) {
      if (t < half) {                            // the step's pairs and their angles
        int pp = t == 0 ? m - 1 : (st + t) % (m - 1);
        int qq = t == 0 ? st % (m - 1) : (st - t + (m - 1)) % (m - 1);
        if (pp > qq) { const int x = pp; pp = qq; qq = x; }
        double c = 1.0, s = 0.0;
        if (qq < k) {
          const double apq = A[pp][qq], app = A[pp][pp], aqq = A[qq][qq];
          if (!(fabs(apq) <= 1e-300 || fabs(apq) <= 1e-18 * sqrt(fabs(app * aqq)))) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double tt = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(tau * tau + 1.0));
            c = 1.0 / sqrt(tt * tt + 1.0); s = tt * c;
          }
        }
        w.rp[t] = pp; w.rq[t] = qq < k ? qq : pp; w.rc[t] = c; w.rsn[t] = s;      // (bye or negligible element: s = 0, skipped below)
      }
      __syncthreads();
      for (int h = wave; h < half; h += NW) {    // A <- A J and V <- V J: the wave takes rotation h, its lanes the rows
        const int pp = w.rp[h], qq = w.rq[h];
        const double c = w.rc[h], s = w.rsn[h];
        if (s == 0.0) continue;                  // wave-uniform
        for (int r = lane; r < k; r += 64) {
          const double arp = A[r][pp], arq = A[r][qq];
          A[r][pp] = c * arp - s * arq;
          A[r][qq] = s * arp + c * arq;
          if constexpr (!Vecs::none) {
            const double vrp = V.at(r, pp), vrq = V.at(r, qq);
            V.at(r, pp) = c * vrp - s * vrq;
            V.at(r, qq) = s * vrp + c * vrq;
          }
        }
      }
      __syncthreads();
      for (int h = wave; h < half; h += NW) {    // A <- J^T A: its lanes the columns
        const int pp = w.rp[h], qq = w.rq[h];
        const double c = w.rc[h], s = w.rsn[h];
        if (s == 0.0) continue;
        for (int r = lane; r < k; r += 64) {
          const double apr = A[pp][r], aqr = A[qq][r];
          A[pp][r] = c * apr - s * aqr;
          A[qq][r] = s * apr + c * aqr;
        }
      }
      __syncthreads();
    }
  }
}

// the same with V [k][k] in LDS, started at the identity here (frechet.hip, geodesic.hip)
template <int KMAX, int NT>
__device__ __forceinline__ void jacobi_lds(double (*A)[KMAX + 1], double (*V)[KMAX + 1], JacobiWs<KMAX>& w, int k) {
  for (int e = threadIdx.x; e < k * k; e += NT) V[e / k][e % k] = (e / k == e % k) ? 1.0 : 0.0;
  __syncthreads();
  jacobi_round_robin<KMAX, NT>(A, JacobiLdsVecs<KMAX>{V}, w, k);
}

// ------------------------------------------------------------------------------------------------------------ streaming helpers
// the sum of v over the workgroup of NT, the same value in every thread; fixed order: xor butterfly, then the waves in order.  red: NT / 64 doubles of LDS
template <int NT>
__device__ inline double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                                  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += red[w];
  return s;
}

// elements n .. n+3 of a row of length N, zeros past its end.  vec: 16-byte accesses are legal (N % 4 == 0, n % 4 == 0 and the row 16-byte aligned, so n + 3 < N)
__device__ inline float4 load4(const float* row, long n, long N, int vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n < N) {
    if (vec) {
      v = *reinterpret_cast<const float4*>(row + n);
    } else {
      v.x = row[n];
      if (n + 1 < N) v.y = row[n + 1];
      if (n + 2 < N) v.z = row[n + 2];
      if (n + 3 < N) v.w = row[n + 3];
    }
  }
  return v;
}

// its mirror: the elements of v that fall inside the row
__device__ inline void store4(float* row, long n, long N, int vec, float4 v) {
  if (n < N) {
    if (vec) {
      *reinterpret_cast<float4*>(row + n) = v;
    } else {
      row[n] = v.x;
      if (n + 1 < N) row[n + 1] = v.y;
      if (n + 2 < N) row[n + 2] = v.z;
      if (n + 3 < N) row[n + 3] = v.w;
    }
  }
}

// Rows cut into slices (chain.hip, hguide.hip): a workgroup of ROW_NT threads takes ROW_SLICE elements of a row, thread t the elements of its
// ROW_GROUPS groups of four in index order; the per-slice fp64 partial sums of a row are then added in slice order.  (noise.hip is NOT one of these:
// its workgroup sum is an LDS halving tree, not block_sum, and the local-PCA goldens pin its bits.)
constexpr int ROW_NT = 256;                 // threads per workgroup
constexpr int ROW_GROUPS = 4;               // groups of four elements per thread and slice
constexpr int ROW_SLICE = ROW_NT * 4 * ROW_GROUPS;   // elements of a row per workgroup: 4096

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// load4 / store4 for group j of a row (j % 4 == 0, j < N) that may start anywhere; al: the row pointer is 16-byte aligned
__device__ inline float4 row_load4(const float* row, long j, long N, bool al) { return load4(row, j, N, al && j + 3 < N); }
__device__ inline void row_store4(float* row, long j, long N, bool al, float4 v) { store4(row, j, N, al && j + 3 < N, v); }

// tot[v] = the sum over a row's nsl slices of part[s][v], slices in index order: one thread's chain, the same in every workgroup of the row
template <int NV>
__device__ inline void sum_slices(const double* part, long nsl, double* tot) {
  double s[NV] = {};
  for (long i = 0; i < nsl; ++i)
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] += part[i * NV + v];
#pragma unroll
  for (int v = 0; v < NV; ++v) tot[v] = s[v];
}

inline long row_slices(long N) { return (N + ROW_SLICE - 1) / ROW_SLICE; }

// n rows of N elements fit a launch: the slices of a row and the rows are grid axes
inline int check_rows(const char* who, long n, long N) {
  if (n < 1 || n > 0x7fffffffL) { set_error("%s: n=%ld rows outside [1, 2^31)", who, n); return -1; }
  if (N < 1) { set_error("%s: row length %ld < 1", who, N); return -1; }
  if (row_slices(N) > 0x7fffffffL) { set_error("%s: row length %ld too large", who, N); return -1; }
  return 0;
}

// bytes of the per-slice partial sums of n rows, two fp64 values per slice; 0 when invalid
inline size_t row_partial_bytes(long n, long N) {
  if (n < 1 || N < 1) return 0;
  return (size_t)n * (size_t)row_slices(N) * 2 * sizeof(double);
}

// One row group of a stream on v_mfma_f64_16x16x4_f64: acc[m][e] += Z[16 m ..][rows r0 .. r0+3] x[rows][column e], Z kept transposed (Zt [rows][k]).
// Lane (j = l & 15, g = l >> 4) holds row r = r0 + g: its coefficients Zt[r][16 m + j] (zero when !rok or past k) and its four loaded columns x, column e
// feeding the MFMAs of tile e.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.
template <int KT>
__device__ __forceinline__ void mfma_rows4(geom_d4 (&acc)[KT][4], const double* Zt, int r, bool rok, int j, int k, const float4& x) {
  double z[KT];
#pragma unroll
  for (int m = 0; m < KT; ++m) z[m] = (rok && 16 * m + j < k) ? Zt[(long)r * k + 16 * m + j] : 0.0;
#pragma unroll
  for (int m = 0; m < KT; ++m) {
    acc[m][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[m], (double)x.x, acc[m][0], 0, 0, 0);
    acc[m][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[m], (double)x.y, acc[m][1], 0, 0, 0);
    acc[m][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[m], (double)x.z, acc[m][2], 0, 0, 0);
    acc[m][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[m], (double)x.w, acc[m][3], 0, 0, 0);
  }
}

}  // namespace dpb
