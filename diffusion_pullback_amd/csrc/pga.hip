// Principal geodesic analysis (tangent PCA) of B local bases of k rows around a base point Y on the Grassmannian -- geometry.grassmann_pga, the analysis of
// run_tangent_space_pga.  It starts where frechet.hip stops: a Frechet scratch block after dpb_frechet_finish holds the whitened Gram Ghat = Q Q^T [R][R],
// the whitenings W_i, the base point's coefficients C (Y = C Q, C Ghat C^T = I) and the canonical rotation Rot of the finish.  Nothing of length N is
// touched until the last pass.
//
// Tangents.  With M_i = Y Q_i^T, I - M_i M_i^T = V sin^2(theta) V^T (Jacobi) and F_i = V theta / (sin cos) V^T (the cosine of a large angle from
// ||(V^T M_i)_t||, as the log map of frechet.hip takes it), E_i = F_i M_i and K_i = F_i M_i M_i^T = V (theta cos / sin) V^T (symmetric),
//   L_i = Log_Y(span Q_i) = E_i Q_i - K_i Y,      row j of L_i the image of row j of Y.
// Since Y Y^T = I and Q_a Y^T = M_a^T (so E_a Q_a Y^T = K_a), the canonical inner product closes in k x k algebra:
//   T_ab = tr(L_a L_b^T) = tr(E_a Ghat_ab E_b^T) - tr(K_a K_b),      T_aa = sum_j theta_aj^2 (written from the angles: no cancellation),
// each pair touching its own k x k block of Ghat only: ONE pass over Ghat, a workgroup per pair a < b, mirrored.  Off the diagonal the two traces are of
// size k and their difference of size theta^2: an absolute error of k 2^-50, nothing for angles above 1e-4 rad.
//
// Analysis.  PCA of the B tangents is the eigen-problem of the centred Gram Tc = H T H (H = I - 1 1^T / B; T itself when not centred): with Tc u = mu u,
// mode = sum_i w_i L_i, w = H u / sqrt(mu) (unit Frobenius norm), variance mu / B, scores sqrt(mu) u_i, residual_i^2 = Tc_ii - sum_m scores_im^2.
// The eigen-solve is the round-robin Jacobi of geom.h in one workgroup while B <= 128 (the matrix in LDS, the vectors in global memory); above that the
// flag-mean solver of flagmean.hip -- block subspace iteration with a Rayleigh-Ritz step -- runs on Tc as a caller's Gram of B one-row "bases".
//
// Synthesis.  A weight row w [B] (a mode, a regression slope, the intercept) gives the tangent sum_i w_i L_i = Zq Q with
//   Zq = (blocks w_i E_i) - (sum_i w_i K_i) C;   Z = (Rot Zq) blockdiag(W)   on the rows of X as given,
// the rotation being the one dpb_frechet_finish applied to Y, so that row j of every output is the image of row j of the returned Y.  All J k output rows
// go through launch_coef_stream, 64 rows per pass over X (fp64 MFMA, rows summed in index order, one rounding).
// A member that is degenerate (flag of the whitening) or whose largest angle to Y exceeds pi/2 - 1e-6 is INVALID: NaN in its row and column of T, left out
// of every statistic and every sum.  Reproducibility: fp64, no atomics, every sum a fixed chain.
#include "kernels.h"
#include "geom.h"

namespace dpb {

constexpr double PGA_HALF_PI = 1.57079632679489661923;
constexpr double PGA_DOMAIN = PGA_HALF_PI - 1e-6;
constexpr int PGA_MAX_MODES = 64;          // the block of the subspace iteration is at most 64 columns wide
constexpr int PGA_MAX_ROWS = 80;           // weight rows of one combine: modes, slopes, the intercept
constexpr int PGA_JACOBI_MAX = 128;        // the B x B fp64 matrix of the one-workgroup eigen-solve lives in LDS
constexpr int PGA_SUBSPACE_ITERS = 200;    // iterations of the subspace route (the launches after convergence are empty)
constexpr double PGA_SUBSPACE_TOL = 1e-13;
constexpr double PGA_DROP = 1e-13;         // an eigenvalue below this share of the largest (or below the rounding floor of T) carries no mode: zero weights

// ------------------------------------------------------------------------------------------------------------ the tangent Gram
// Out^T [R][k] = Ghat In^T as fr_product_kernel forms it, with the rows of degenerate members left out of the sum (their blocks of Ghat are NaN, and
// 0 * NaN would spoil every member): the columns of a degenerate member still come out NaN.
template <int KT>
__global__ __launch_bounds__(256) void pga_product_kernel(const double* G, const double* In, const int* flags, double* Out, int R, int k) {
  __shared__ double red[4][KT][4][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * 16;
  const int steps = (R + 3) / 4, q = (steps + 3) / 4;
  const int s0 = wave * q, s1 = s0 + q < steps ? s0 + q : steps;
  geom_d4 acc[KT];
#pragma unroll
  for (int m = 0; m < KT; ++m) acc[m] = geom_d4{0.0, 0.0, 0.0, 0.0};
  const bool cok = c0 + j < R;
  for (int s = s0; s < s1; ++s) {
    const int r = 4 * s + g;
    const bool rok = r < R && flags[r / k] == 0;
    const double a = (rok && cok) ? G[(long)r * R + c0 + j] : 0.0;
#pragma unroll
    for (int m = 0; m < KT; ++m) {
      const int col = 16 * m + j;
      const double b = (rok && col < k) ? In[(long)r * k + col] : 0.0;
      acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[m], 0, 0, 0);
    }
  }
#pragma unroll
  for (int m = 0; m < KT; ++m)
#pragma unroll
    for (int x = 0; x < 4; ++x) red[wave][m][x][lane] = acc[m][x];
  __syncthreads();
  for (int e = t; e < KT * 4 * 64; e += 256) {
    const int m = e / 256, x = (e >> 6) & 3, ln = e & 63;
    const double v = ((red[0][m][x][ln] + red[1][m][x][ln]) + red[2][m][x][ln]) + red[3][m][x][ln];
    const int c = c0 + (ln >> 4) + 4 * x, a = 16 * m + (ln & 15);
    if (c < R && a < k) Out[(long)c * k + a] = v;
  }
}

// One workgroup per member i: from block i of Mt (M_i transposed) the angles (fp32, descending), T_ii = sum theta^2, the state (bit 0 degenerate, bit 1
// outside the log map's domain, bit 2 otherwise not finite), E_i = F_i M_i transposed (element b k + a = E_i[a][b]) and K_i; NaN for an invalid member
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void pga_member_kernel(const double* Mt, const int* flags, double* Et, double* Kk, float* theta, double* diag, int* state, int k) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], Mm[KMAX][KMAX + 1];
  __shared__ double lam[KMAX], thr[KMAX], ths[KMAX], fv[KMAX], hv[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  __shared__ int bad;
  static_assert(sizeof(double) * (3 * KMAX * (KMAX + 1) + 5 * KMAX) + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "pga_member_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  const long i = blockIdx.x;
  const double* Mb = Mt + i * k * k;
  for (int e = t; e < k * k; e += NT) Mm[e % k][e / k] = Mb[e];
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {            // S = I - M M^T, the upper half mirrored
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0;
      for (int b = 0; b < k; ++b) s += Mm[r][b] * Mm[c][b];
      const double v = (r == c ? 1.0 : 0.0) - s;
      A[r][c] = v; A[c][r] = v;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(A, V, ws, k);
  if (t < k) {
    const double l = A[t][t];
    lam[t] = l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);  // (a NaN stays a NaN)
  }
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {            // U = V^T M into A: row t has norm cos(theta_t)
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b < k; ++b) s += V[b][r] * Mm[b][c];
    A[r][c] = s;
  }
  __syncthreads();
  if (t < k) {                                     // the angle rule of fr_basis_kernel
    const double l = lam[t];
    double sn, cs, th;
    if (l <= 0.5) {
      sn = sqrt(l); cs = sqrt(1.0 - l); th = asin(sn);
    } else {
      double c2 = 0.0;
      for (int b = 0; b < k; ++b) c2 += A[t][b] * A[t][b];
      c2 = c2 > 1.0 ? 1.0 : c2;
      cs = sqrt(c2); sn = sqrt(1.0 - c2); th = acos(cs);
    }
    thr[t] = th;
    fv[t] = sn > 0.0 ? th / (sn * cs) : (sn == 0.0 ? 1.0 : sn);
    hv[t] = sn > 0.0 ? th * cs / sn : (sn == 0.0 ? 1.0 : sn);
  }
  __syncthreads();
  if (t < k) ths[rank_desc(thr, k, t)] = thr[t];
  __syncthreads();
  for (int e = t; e < k; e += NT) theta[i * k + e] = (float)ths[e];
  if (t == 0) {
    double s = 0.0;
    for (int e = 0; e < k; ++e) s += ths[e] * ths[e];
    int st = flags[i] ? 1 : 0;
    if (!st && ths[0] > PGA_DOMAIN) st = 2;
    if (!st && !(s == s && s < 1e300)) st = 4;
    state[i] = st;
    diag[i] = st ? nan64() : s;
    bad = st;
  }
  __syncthreads();
  const bool inv = bad != 0;
  double* Eb = Et + i * k * k;
  double* Kb = Kk + i * k * k;
  for (int e = t; e < k * k; e += NT) {            // (F M)[a][b] = sum_x V[a][x] f_x U[x][b], stored transposed
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int x = 0; x < k; ++x) s += V[a][x] * fv[x] * A[x][b];
    Eb[e] = inv ? nan64() : s;
  }
  for (int e = t; e < k * k; e += NT) {            // K_i = V h V^T, the upper half mirrored
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0;
      for (int x = 0; x < k; ++x) s += V[r][x] * hv[x] * V[c][x];
      s = inv ? nan64() : s;
      Kb[r * k + c] = s; Kb[c * k + r] = s;
    }
  }
}

// One workgroup per pair a <= b: T_ab = sum_{r,c} (E_a Ghat_ab)[r][c] E_b[r][c] - sum K_a[r][c] K_b[r][c], mirrored.  E_a (transposed) and the pair's block of
// Ghat sit in LDS; the k^2 terms are summed per thread in index order, then over the workgroup in the fixed order of block_sum.
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void pga_pair_kernel(const double* G, const double* Et, const double* Kk, const double* diag, const int* state, double* T,
                                                      int n, int R, int k) {
  const int a = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  if (a > b) return;
  if (a == b) { if (t == 0) T[(long)a * n + a] = diag[a]; return; }
  if (state[a] || state[b]) { if (t == 0) { T[(long)a * n + b] = nan64(); T[(long)b * n + a] = nan64(); } return; }
  __shared__ double Ea[KMAX][KMAX + 1], Gb[KMAX][KMAX + 1], red[NT / 64];
  const double* Eap = Et + (long)a * k * k;
  const double* Ebp = Et + (long)b * k * k;
  const double* Kap = Kk + (long)a * k * k;
  const double* Kbp = Kk + (long)b * k * k;
  const double* Gab = G + ((long)a * k) * R + (long)b * k;
  for (int e = t; e < k * k; e += NT) {
    Ea[e / k][e % k] = Eap[e];                     // Ea[x][r] = E_a[r][x]
    Gb[e / k][e % k] = Gab[(long)(e / k) * R + e % k];
  }
  __syncthreads();
  double acc = 0.0;
  for (int e = t; e < k * k; e += NT) {
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int x = 0; x < k; ++x) s += Ea[x][r] * Gb[x][c];
    acc += s * Ebp[c * k + r] - Kap[e] * Kbp[e];
  }
  const double v = block_sum<NT>(acc, red);
  if (t == 0) { T[(long)a * n + b] = v; T[(long)b * n + a] = v; }
}

// ------------------------------------------------------------------------------------------------------------ the eigen-problem
// a member is valid when its diagonal entry of T is a number
__device__ inline bool pga_ok(const double* T, int n, int i) { const double d = T[(long)i * n + i]; return d == d; }

// row i: rs[i] = the sum of T_ij over the valid j (0 for an invalid i)
__global__ __launch_bounds__(256) void pga_rowsum_kernel(const double* T, double* rs, int n) {
  __shared__ double red[4];
  const int i = blockIdx.x, t = threadIdx.x;
  const bool vi = pga_ok(T, n, i);
  double s = 0.0;
  if (vi)
    for (int j = t; j < n; j += 256)
      if (pga_ok(T, n, j)) s += T[(long)i * n + j];
  s = block_sum<256>(s, red);
  if (t == 0) rs[i] = vi ? s : 0.0;
}

// one workgroup: hd[0] = the number of valid members, hd[1] = 1^T T 1 over them
__global__ __launch_bounds__(256) void pga_head_kernel(const double* T, const double* rs, double* hd, int n) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double c = 0.0, s = 0.0;
  for (int i = t; i < n; i += 256)
    if (pga_ok(T, n, i)) { c += 1.0; s += rs[i]; }
  c = block_sum<256>(c, red);
  s = block_sum<256>(s, red);
  if (t == 0) { hd[0] = c; hd[1] = s; }
}

// row i of Tc = H T H over the valid members (center) or T itself, the rows and columns of invalid members zero
__global__ __launch_bounds__(256) void pga_center_kernel(const double* T, const double* rs, const double* hd, double* Tc, int n, int center) {
  const int i = blockIdx.x;
  const double nv = hd[0], grand = hd[1];
  const bool vi = pga_ok(T, n, i);
  for (int j = threadIdx.x; j < n; j += 256) {
    double v = 0.0;
    if (vi && pga_ok(T, n, j)) {
      v = T[(long)i * n + j];
      if (center) v = (v - (rs[i] + rs[j]) / nv) + grand / (nv * nv);
    }
    Tc[(long)i * n + j] = v;
  }
}

// one workgroup: Tc = V diag(lam) V^T by the round-robin Jacobi of geom.h, the matrix in LDS, the vectors transposed in global memory (Vt [n][n]);
// the first M eigenvalues in descending order into evals, their unit vectors into evec [M][n]
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void pga_jacobi_kernel(const double* Tc, double* Vt, double* evals, double* evec, int n, int M) {
  __shared__ double A[KMAX][KMAX + 1], lam[KMAX];
  __shared__ int sel[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (KMAX * (KMAX + 1) + KMAX) + sizeof(int) * KMAX + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "pga_jacobi_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  for (int e = t; e < n * n; e += NT) {
    A[e / n][e % n] = Tc[e];
    Vt[e] = (e / n == e % n) ? 1.0 : 0.0;
  }
  __syncthreads();
  jacobi_round_robin<KMAX, NT>(A, JacobiGlobalVecsT{Vt, n}, ws, n);
  if (t < n) lam[t] = A[t][t];
  __syncthreads();
  if (t < n) {
    const int rk = rank_desc(lam, n, t);
    sel[rk] = t;
  }
  __syncthreads();
  for (int e = t; e < M; e += NT) evals[e] = lam[sel[e]];
  for (int e = t; e < M * n; e += NT) evec[e] = Vt[(long)sel[e / n] * n + e % n];
}

// the subspace route's answer in the same form: evec[m][i] = Ct[i][m], evals[m] = the Ritz values of the flag-mean finish (info[8 + m])
__global__ __launch_bounds__(256) void pga_pack_kernel(const double* Ct, const double* info, double* evals, double* evec, int n, int M) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < (long)M * n) evec[e] = Ct[(e % n) * M + e / n];
  if (e < M) evals[e] = info[8 + e];
}

// one workgroup: per mode the unit eigenvector, the sign rule (the largest-magnitude score positive; magnitudes within 1e-9 of it tie, the lowest member wins), the weights on the
// tangents, the scores; then the residuals and the header.  out: [0] valid members, [1] total variance, [2] ||mean tangent||, [3] route, [4] / [5] the
// subspace solver's iterations / status, [8 .. 72) variance, scores [n][M], residual [n]
__global__ __launch_bounds__(256) void pga_post_kernel(const double* T, const double* Tc, const double* hd, const double* evals, const double* evec,
                                                       const double* finfo, double* Wt, double* out, int n, int M, int center, int route, double floor) {
  __shared__ double red[4], bv[256];
  __shared__ int bi[256];
  __shared__ double sgs;
  const int t = threadIdx.x;
  const double nv = hd[0];
  double* var = out + 8;
  double* scores = out + 72;
  double* resid = scores + (long)n * M;
  const double mu0 = evals[0];
  for (int e = t; e < 64; e += 256) var[e] = 0.0;
  for (int m = 0; m < M; ++m) {
    const double* u = evec + (long)m * n;
    const double mu = evals[m];
    double s2 = 0.0, s1 = 0.0;
    for (int i = t; i < n; i += 256)
      if (pga_ok(T, n, i)) { s2 += u[i] * u[i]; s1 += u[i]; }
    s2 = block_sum<256>(s2, red);
    s1 = block_sum<256>(s1, red);
    const bool live = nv > 0.0 && mu > floor && mu > PGA_DROP * mu0 && s2 > 0.0;
    const double inv = live ? 1.0 / sqrt(s2) : 0.0;
    double best = 0.0;                             // the largest magnitude, then the lowest member within 1e-9 of it: a tie in exact arithmetic stays one
    for (int i = t; i < n; i += 256)
      if (pga_ok(T, n, i)) { const double a = fabs(u[i]); if (a > best) best = a; }
    bv[t] = best;
    __syncthreads();
    if (t == 0) {
      double b = 0.0;
      for (int e = 0; e < 256; ++e) b = bv[e] > b ? bv[e] : b;
      sgs = b;
    }
    __syncthreads();
    const double cut = sgs * (1.0 - 1e-9);
    int idx = n;
    for (int i = t; i < n; i += 256)
      if (pga_ok(T, n, i) && fabs(u[i]) >= cut) { idx = i; break; }
    bi[t] = idx;
    __syncthreads();
    if (t == 0) {
      int ix = n;
      for (int e = 0; e < 256; ++e) ix = bi[e] < ix ? bi[e] : ix;
      sgs = (ix < n && u[ix] < 0.0) ? -1.0 : 1.0;
      var[m] = live ? mu / nv : 0.0;
    }
    __syncthreads();
    const double sg = sgs, rt = live ? sqrt(mu) : 0.0, ubar = (live && center) ? s1 * inv / nv : 0.0;
    for (int i = t; i < n; i += 256) {
      const bool ok = pga_ok(T, n, i);
      const double ui = ok ? sg * u[i] * inv : 0.0;
      Wt[(long)m * n + i] = (ok && live) ? (ui - sg * ubar) / rt : 0.0;
      scores[(long)i * M + m] = ok ? rt * ui : nan64();
    }
    __syncthreads();
  }
  double tr = 0.0;
  for (int i = t; i < n; i += 256) {
    const bool ok = pga_ok(T, n, i);
    const double d = Tc[(long)i * n + i];
    if (ok) tr += d;
    double s = 0.0;
    for (int m = 0; m < M; ++m) { const double v = scores[(long)i * M + m]; s += v * v; }
    const double r2 = d - s;
    resid[i] = ok ? sqrt(r2 > 0.0 ? r2 : 0.0) : nan64();
  }
  tr = block_sum<256>(tr, red);
  if (t == 0) {
    out[0] = nv;
    out[1] = nv > 0.0 ? (tr > 0.0 ? tr : 0.0) / nv : 0.0;
    out[2] = nv > 0.0 ? sqrt(hd[1] > 0.0 ? hd[1] : 0.0) / nv : 0.0;
    out[3] = (double)route;
    out[4] = route == 2 ? finfo[0] : 0.0;
    out[5] = route == 2 ? finfo[1] : 0.0;
    out[6] = 0.0; out[7] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------------------ synthesis
// weight row j: Ks[j] = sum_i w_ji K_i over the valid members in index order
__global__ __launch_bounds__(256) void pga_ksum_kernel(const double* Wt, const double* Kk, const int* state, double* Ks, int n, int k) {
  const long j = blockIdx.x;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    double s = 0.0;
    for (long i = 0; i < n; ++i)
      if (state[i] == 0) s += Wt[j * n + i] * Kk[i * k * k + e];
    Ks[j * k * k + e] = s;
  }
}

// block i of weight row j: Zq = w_ji E_i - Ks_j C_i (k x k, on the whitened rows of member i), rotated as the finish rotated Y and carried to the rows of X
// by W_i; stored transposed into the pass that holds output row j k + a: pass g = (j k + a) / 64 is a matrix [R][kg], kg = min(64, J k - 64 g), at
// offset 64 g R.  A degenerate member's rows take no part (zeros)
template <int KMAX>
__global__ __launch_bounds__(256) void pga_coef_kernel(const double* Wt, const double* Et, const double* Ks, const double* Ct, const double* Rot, const double* W,
                                                       const int* flags, const int* state, double* Zt, int n, int R, int k, int J) {
  __shared__ double Zq[KMAX][KMAX + 1], Cp[KMAX][KMAX + 1];
  const long i = blockIdx.x, j = blockIdx.y;
  const int t = threadIdx.x;
  const long base = i * k * k;
  const bool member = i < n && state[i] == 0;
  const double w = member ? Wt[j * n + i] : 0.0;
  const double* Ksj = Ks + j * k * k;
  for (int e = t; e < k * k; e += 256) {
    const int c = e / k, b = e % k;                // Zq[c][b]
    double s = 0.0;
    for (int x = 0; x < k; ++x) s += Ksj[c * k + x] * Ct[base + b * k + x];
    Zq[c][b] = (member ? w * Et[base + b * k + c] : 0.0) - s;
  }
  __syncthreads();
  for (int e = t; e < k * k; e += 256) {
    const int a = e / k, b = e % k;
    double s = 0.0;
    for (int c = 0; c < k; ++c) s += Rot[a * k + c] * Zq[c][b];
    Cp[a][b] = s;
  }
  __syncthreads();
  const double* Wi = W + base;
  const bool bad = flags[i] != 0;
  const long rows = (long)J * k;
  for (int e = t; e < k * k; e += 256) {
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int c = b; c < k; ++c) s += Cp[a][c] * Wi[c * k + b];
    const long o = j * k + a, g = o / 64;
    const long kg = rows - 64 * g < 64 ? rows - 64 * g : 64;
    Zt[64 * g * R + (i * k + b) * kg + o % 64] = bad ? 0.0 : s;
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
namespace {
struct PgaLayout {
  size_t state = 0, diag = 0, Et = 0, Kk = 0, Mt = 0, rs = 0, hd = 0, Tc = 0, Vt = 0, evals = 0, evec = 0, solver = 0, fCt = 0, finfo = 0, ftheta = 0, fweight = 0,
         Ks = 0, Zt = 0, total = 0, solver_bytes = 0;
};
bool pga_layout(long B, long n, int k, long N, int J, PgaLayout& l) {
  if (frechet_scratch_bytes(B, k, N, 0) == 0 || n < 1 || n > B || n < B - 1 || J < 1 || J > PGA_MAX_ROWS) return false;
  const int r = (int)(n < PGA_MAX_MODES ? n : PGA_MAX_MODES);
  l.solver_bytes = flag_mean_scratch_bytes(n, 1, N, r, PGA_SUBSPACE_ITERS, false);
  if (l.solver_bytes == 0) return false;
  ScratchCarver s;
  const size_t R = (size_t)B * k, kk = (size_t)k * k * sizeof(double), nn = (size_t)n * n * sizeof(double);
  l.state = s.take((size_t)n * sizeof(int));
  l.diag = s.take((size_t)n * sizeof(double));
  l.Et = s.take((size_t)n * kk);
  l.Kk = s.take((size_t)n * kk);
  l.Mt = s.take(R * k * sizeof(double));
  l.rs = s.take((size_t)n * sizeof(double));
  l.hd = s.take(8 * sizeof(double));
  l.Tc = s.take(nn);
  l.Vt = s.take(n <= PGA_JACOBI_MAX ? nn : 0);
  l.evals = s.take(PGA_MAX_MODES * sizeof(double));
  l.evec = s.take((size_t)PGA_MAX_MODES * n * sizeof(double));
  l.solver = s.take(l.solver_bytes);
  l.fCt = s.take((size_t)n * PGA_MAX_MODES * sizeof(double));
  l.finfo = s.take((72 + (size_t)n) * sizeof(double));
  l.ftheta = s.take((size_t)n * sizeof(float));
  l.fweight = s.take(PGA_MAX_MODES * sizeof(float));
  l.Ks = s.take((size_t)J * kk);
  l.Zt = s.take(R * (size_t)J * k * sizeof(double));
  l.total = s.off;
  return true;
}
int pga_check(const char* who, long B, long n, int k, long N, int J, const void* scratch, size_t scratch_bytes, PgaLayout& l) {
  if (!pga_layout(B, n, k, N, J, l)) {
    set_error("%s: B=%ld, k=%d (at most %d), N=%ld is no Frechet problem, members=%ld outside [max(1,B-1),B], or J=%d outside [1,%d]", who, B, k, FRECHET_MAX_RANK,
              N, n, J, PGA_MAX_ROWS);
    return -1;
  }
  return check_scratch(who, scratch, scratch_bytes, l.total, "dpb_pga_scratch_bytes(%ld, %ld, %d, %ld, %d)", B, n, k, N, J);
}
int g_pga_route = 0;      // dpb_debug_set("pga_route", v): 0 by size, 1 the one-workgroup Jacobi (B <= 128 only), 2 the subspace iteration
}  // namespace

void pga_debug_route(int v) { g_pga_route = v; }

size_t pga_scratch_bytes(long B, long n, int k, long N, int J) {
  PgaLayout l;
  return pga_layout(B, n, k, N, J, l) ? l.total : 0;
}

int launch_pga_tangent_gram(long B, long n, int k, long N, long max_iter, int J, void* fscratch, size_t fbytes, double* T, float* theta, int32_t* state,
                            void* scratch, size_t scratch_bytes, hipStream_t st) {
  PgaLayout l;
  if (pga_check("dpb_pga_tangent_gram", B, n, k, N, J, scratch, scratch_bytes, l) != 0) return -1;
  FrechetView f;
  if (!frechet_view(B, k, N, max_iter, fscratch, f)) { set_error("dpb_pga_tangent_gram: B=%ld, k=%d, N=%ld, max_iter=%ld is no Frechet problem", B, k, N, max_iter); return -1; }
  if (check_scratch("dpb_pga_tangent_gram", fscratch, fbytes, f.total, "dpb_frechet_scratch_bytes(%ld, %d, %ld, %ld)", B, k, N, max_iter) != 0) return -1;
  char* b = (char*)scratch;
  int* sta = (int*)(b + l.state);
  double *diag = (double*)(b + l.diag), *Et = (double*)(b + l.Et), *Kk = (double*)(b + l.Kk), *Mt = (double*)(b + l.Mt);
  const int R = (int)(B * k), nn = (int)n;
  DPB_BY_TILES(k, DPB_LAUNCH((pga_product_kernel<KT>), dim3((R + 15) / 16), dim3(256), 0, st, f.G, f.Ct, f.flags, Mt, R, k));
  DPB_BY_RANK(k, DPB_LAUNCH((pga_member_kernel<KM, NT>), dim3((unsigned)n), dim3(NT), 0, st, Mt, f.flags, Et, Kk, theta, diag, sta, k));
  const dim3 gp((unsigned)n, (unsigned)n);
  DPB_BY_RANK(k, DPB_LAUNCH((pga_pair_kernel<KM, NT>), gp, dim3(NT), 0, st, f.G, Et, Kk, diag, sta, T, nn, R, k));
  DPB_CHECK(hipMemcpyAsync(state, sta, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_pga_eig(const double* T, long B, long n, int k, long N, int J, int M, int center, double* Wt, double* out, void* scratch, size_t scratch_bytes,
                   hipStream_t st) {
  PgaLayout l;
  if (pga_check("dpb_pga_eig", B, n, k, N, J, scratch, scratch_bytes, l) != 0) return -1;
  if (M < 1 || M > PGA_MAX_MODES || M > n || M > J) { set_error("dpb_pga_eig: M=%d outside [1,min(%d,members=%ld,J=%d)]", M, PGA_MAX_MODES, n, J); return -1; }
  if (g_pga_route == 1 && n > PGA_JACOBI_MAX) { set_error("dpb_pga_eig: the Jacobi route takes at most %d members, got %ld", PGA_JACOBI_MAX, n); return -1; }
  char* b = (char*)scratch;
  double *rs = (double*)(b + l.rs), *hd = (double*)(b + l.hd), *Tc = (double*)(b + l.Tc), *Vt = (double*)(b + l.Vt), *evals = (double*)(b + l.evals),
         *evec = (double*)(b + l.evec), *fCt = (double*)(b + l.fCt), *finfo = (double*)(b + l.finfo);
  const int nn = (int)n;
  const dim3 gn((unsigned)n), one(1), t256(256);
  DPB_LAUNCH(pga_rowsum_kernel, gn, t256, 0, st, T, rs, nn);
  DPB_LAUNCH(pga_head_kernel, one, t256, 0, st, T, rs, hd, nn);
  DPB_LAUNCH(pga_center_kernel, gn, t256, 0, st, T, rs, hd, Tc, nn, center ? 1 : 0);
  const int route = g_pga_route == 2 || n > PGA_JACOBI_MAX ? 2 : 1;
  if (route == 1) {
    DPB_BY_RANK128(nn, DPB_LAUNCH((pga_jacobi_kernel<KM, NT>), one, dim3(NT), 0, st, Tc, Vt, evals, evec, nn, M));
  } else {
    void* fs = b + l.solver;
    if (launch_flag_mean_init(nullptr, Tc, n, 1, N, M, 0ULL, PGA_SUBSPACE_ITERS, fs, l.solver_bytes, st) != 0) return -1;
    if (launch_flag_mean_iterate(Tc, n, 1, N, M, PGA_SUBSPACE_ITERS, PGA_SUBSPACE_ITERS, PGA_SUBSPACE_TOL, fs, l.solver_bytes, st) != 0) return -1;
    if (launch_flag_mean_finish(nullptr, Tc, n, 1, N, M, PGA_SUBSPACE_ITERS, nullptr, (float*)(b + l.fweight), (float*)(b + l.ftheta), fCt, finfo, fs,
                                l.solver_bytes, st) != 0) return -1;
    DPB_LAUNCH(pga_pack_kernel, dim3((unsigned)(((long)M * n + 255) / 256)), t256, 0, st, fCt, finfo, evals, evec, nn, M);
  }
  // entries of T carry an absolute error near k 2^-50 (the header): an eigenvalue of Tc below members k 2^-46 is rounding, not a mode
  DPB_LAUNCH(pga_post_kernel, one, t256, 0, st, T, Tc, hd, evals, evec, finfo, Wt, out, nn, M, center ? 1 : 0, route, (double)n * k * 0x1p-46);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_pga_combine(const float* X, const double* Wt, long B, long n, int k, long N, long max_iter, int J, int Jw, void* fscratch, size_t fbytes, float* out,
                       void* scratch, size_t scratch_bytes, hipStream_t st) {
  PgaLayout l;
  if (pga_check("dpb_pga_combine", B, n, k, N, J, scratch, scratch_bytes, l) != 0) return -1;
  if (Jw < 1 || Jw > J) { set_error("dpb_pga_combine: %d weight rows outside [1,J=%d]", Jw, J); return -1; }
  FrechetView f;
  if (!frechet_view(B, k, N, max_iter, fscratch, f)) { set_error("dpb_pga_combine: B=%ld, k=%d, N=%ld, max_iter=%ld is no Frechet problem", B, k, N, max_iter); return -1; }
  if (check_scratch("dpb_pga_combine", fscratch, fbytes, f.total, "dpb_frechet_scratch_bytes(%ld, %d, %ld, %ld)", B, k, N, max_iter) != 0) return -1;
  char* b = (char*)scratch;
  const int* sta = (const int*)(b + l.state);
  const double *Et = (const double*)(b + l.Et), *Kk = (const double*)(b + l.Kk);
  double *Ks = (double*)(b + l.Ks), *Zt = (double*)(b + l.Zt);
  const int R = (int)(B * k), nn = (int)n;
  DPB_LAUNCH(pga_ksum_kernel, dim3((unsigned)Jw), dim3(256), 0, st, Wt, Kk, sta, Ks, nn, k);
  const dim3 gc((unsigned)B, (unsigned)Jw);
  DPB_BY_RANK(k, (void)NT; DPB_LAUNCH((pga_coef_kernel<KM>), gc, dim3(256), 0, st, Wt, Et, Ks, f.Ct, f.Rot, f.W, f.flags, sta, Zt, nn, R, k, Jw));
  const long rows = (long)Jw * k;
  for (long g = 0; 64 * g < rows; ++g) {
    const int kg = (int)(rows - 64 * g < 64 ? rows - 64 * g : 64);
    if (launch_coef_stream(X, Zt + 64 * g * R, out + 64 * g * N, R, kg, N, st) != 0) return -1;
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
