// The two-sided Jacobi eigen-solve with eigenvectors shared by the Frechet mean (frechet.hip) and the Grassmann geodesics (geodesic.hip).
#pragma once
#include "kernels.h"

namespace dpb {

// A [k][k] symmetric in LDS -> diagonal, V its eigenvectors in columns (A_in = V diag V^T): two-sided Jacobi in the round-robin order, floor(k/2) disjoint
// rotations per step, the ordering and thresholds of the eigen-solves of angles.hip / orth.hip.  Every thread of the workgroup calls it.
template <int KMAX>
struct FrJacobiWs {
  double rc[KMAX / 2 + 1], rsn[KMAX / 2 + 1], red[2][16];
  int rp[KMAX / 2 + 1], rq[KMAX / 2 + 1];
};

template <int KMAX, int NT>
__device__ void fr_jacobi(double (*A)[KMAX + 1], double (*V)[KMAX + 1], FrJacobiWs<KMAX>& w, int k) {
  constexpr int NW = NT / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int e = t; e < k * k; e += NT) V[e / k][e % k] = (e / k == e % k) ? 1.0 : 0.0;
  __syncthreads();
  const int m = (k + 1) & ~1, half = m / 2, steps = m - 1;      // players 0 .. m-1 (player k is a bye when k is odd)
  for (int sweep = 0; sweep < 30 && k > 1; ++sweep) {
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
          const double vrp = V[r][pp], vrq = V[r][qq];
          V[r][pp] = c * vrp - s * vrq;
          V[r][qq] = s * vrp + c * vrq;
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
  __syncthreads();
}

}  // namespace dpb
