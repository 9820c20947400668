// Frechet (Karcher) mean on the Grassmannian of B local bases of k rows in R^N -- the global basis of run_edit_global_frechet_mean_zt (src/modules/edit.py:951-1246;
// the reference hands the problem to pymanopt).  X [B][k][N] fp32, rows need not be orthonormal; R = B k.
//
// Nothing of size N is touched while the mean iterates.  With Q_i = W_i X_i the orthonormalised bases (W_i: the whitening of angles.hip) every iterate
// lies in the span of the R rows, Y = C Q with C [k][R], and all the Riemannian arithmetic needs is the whitened Gram Ghat = Q Q^T [R][R]:
//   M = C Ghat, block i: M_i = Y Q_i^T;   S_i = I - M_i M_i^T = V sin^2(theta) V^T (Jacobi);   Log_Y(Q_i) = F_i (M_i Q_i - M_i M_i^T Y), F_i = V f(theta) V^T,
//   f = theta / (sin cos) (the cosine of an angle above pi/4 from ||(V^T M_i)_t||, not from 1 - sin^2);   mean tangent T = C_T Q, C_T = (blocks F_i M_i - (sum_i F_i M_i M_i^T) C) / B;   T T^T = (C_T Ghat) C_T^T = P Sigma^2 P^T (Jacobi);
//   C <- P cos(tau Sigma) P^T C + P sin(tau Sigma) / Sigma P^T C_T, then whitened by the Cholesky factor of its own Gram C Ghat C^T.
// One pass over X forms G (dpb_cross_gram, exact products) before the iteration; one pass forms Y = (C blockdiag(W)) X after it, on the fp64 matrix cores with
// the fp32 rows widened on load, summed over the rows in index order and rounded once.
// All coefficient matrices are kept TRANSPOSED, [R][k] (row r = one of the R rows, k coefficients next to each other): block i is then a contiguous k x k piece.
// Reproducibility: fp64, no atomics, every sum a fixed chain -- the r range of a product is cut among the four waves of a workgroup at bounds that depend
// on R only and the four partial sums are added in wave order; sums over the bases run in index order.  A step reads and writes device state only, so
// iterate(a) then iterate(b) is bitwise iterate(a + b).
#include "kernels.h"
#include "geom.h"

namespace dpb {

struct FrCtl {            // the first bytes of the scratch block (documented in dpb.h: the caller may read them)
  int done;               // 0 running, 1 converged (g < tol), 2 a basis left the log map's domain, 3 the history is full
  int domain;             // the basis that left the domain, or -1
  int iters;              // Karcher steps taken
  int reorth_bad;         // the re-orthonormalisation met a non-positive pivot (NaN coefficients follow)
  double g, cost;         // the last gradient norm and cost computed
};

constexpr double FR_HALF_PI = 1.57079632679489661923;
constexpr double FR_DOMAIN = FR_HALF_PI - 1e-6;      // a largest principal angle beyond this is outside the log map's domain

// ------------------------------------------------------------------------------------------------------------ init
// block (i, j), i <= j, of G in place: Ghat_ij = W_i G_ij W_j^T, mirrored into (j, i); the diagonal blocks are the identity; a degenerate basis's blocks NaN
template <int KMAX>
__global__ __launch_bounds__(256) void fr_whiten_kernel(double* G, const double* W, const int* flags, int R, int k) {
  const int i = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
  if (i > j) return;
  __shared__ double Gb[KMAX][KMAX + 1], Tb[KMAX][KMAX + 1];
  double* Gij = G + ((long)i * k) * R + (long)j * k;
  double* Gji = G + ((long)j * k) * R + (long)i * k;
  if (flags[i] || flags[j]) {
    for (int e = t; e < k * k; e += 256) { Gij[(long)(e / k) * R + e % k] = nan64(); Gji[(long)(e % k) * R + e / k] = nan64(); }
    return;
  }
  if (i == j) {
    for (int e = t; e < k * k; e += 256) Gij[(long)(e / k) * R + e % k] = (e / k == e % k) ? 1.0 : 0.0;
    return;
  }
  const double* Wi = W + (long)i * k * k;
  const double* Wj = W + (long)j * k * k;
  for (int e = t; e < k * k; e += 256) Gb[e / k][e % k] = Gij[(long)(e / k) * R + e % k];
  __syncthreads();
  for (int e = t; e < k * k; e += 256) {           // T = W_i G_ij (W_i lower triangular)
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b <= r; ++b) s += Wi[r * k + b] * Gb[b][c];
    Tb[r][c] = s;
  }
  __syncthreads();
  for (int e = t; e < k * k; e += 256) {           // Ghat_ij = T W_j^T
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b <= c; ++b) s += Tb[r][b] * Wj[c * k + b];
    Gij[(long)r * R + c] = s;
    Gji[(long)c * R + r] = s;
  }
}

// C = the identity in block `init` (transposed storage), the control block cleared
__global__ __launch_bounds__(256) void fr_init_kernel(double* Ct, FrCtl* ctl, int R, int k, int init) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < (long)R * k) Ct[e] = (e / k == (long)init * k + e % k) ? 1.0 : 0.0;
  if (e == 0) { ctl->done = 0; ctl->domain = -1; ctl->iters = 0; ctl->reorth_bad = 0; ctl->g = 0.0; ctl->cost = 0.0; }
}

// dpb_frechet_start: the caller's coefficients into Cn and the status cleared (phase 0); the step count cleared again after the whitening (phase 1)
__global__ __launch_bounds__(256) void fr_start_kernel(const double* src, double* Cn, FrCtl* ctl, long n, int phase) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) Cn[e] = src[e];
  if (e == 0) {
    ctl->iters = 0;
    if (phase == 0) { ctl->done = 0; ctl->domain = -1; ctl->reorth_bad = 0; ctl->g = 0.0; ctl->cost = 0.0; }
  }
}

// ------------------------------------------------------------------------------------------------------------ the skinny product with Ghat
// Out^T [R][k] = Ghat [R][R] In^T [R][k] (that is Out = In Ghat, Ghat symmetric) on v_mfma_f64_16x16x4_f64.  A workgroup owns 16 rows of Out^T and reads
// the matching 16-column strip of Ghat once (128 contiguous bytes per row; by symmetry Ghat[c][r] is read as Ghat[r][c]); its four waves take a quarter of
// the r range each and their partial tiles are added in wave order.  Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; C/D of the f64
// MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.
template <int KT>
__global__ __launch_bounds__(256) void fr_product_kernel(const double* G, const double* In, double* Out, int R, int k, const FrCtl* ctl, int force) {
  if (!force && ctl->done) return;
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
    const bool rok = r < R;
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

// ------------------------------------------------------------------------------------------------------------ per basis: the log map
// One workgroup per basis i.  Mt block i holds M_i transposed.  mode 0 (a Karcher step; a no-op once done): theta_i, the cost term, the domain flag, the raw
// tangent coefficients F_i M_i into block i of FMt, and H_i = F_i M_i M_i^T = V (theta cos / sin) V^T into Ps[i].  mode 1 (finish): theta_i, the cost term
// and M_i M_i^T into Ps[i].
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fr_basis_kernel(const double* Mt, double* FMt, double* Ps, double* thetas, double* costs, int* dom, const FrCtl* ctl,
                                                      int k, int mode) {
  if (mode == 0 && ctl->done) return;
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], Mm[KMAX][KMAX + 1];
  __shared__ double lam[KMAX], thr[KMAX], ths[KMAX], fv[KMAX], hv[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (3 * KMAX * (KMAX + 1) + 5 * KMAX) + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "fr_basis_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  const long i = blockIdx.x;
  const double* Mb = Mt + i * k * k;
  double* Pi = Ps + i * k * k;
  for (int e = t; e < k * k; e += NT) Mm[e % k][e / k] = Mb[e];
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {            // S = I - M M^T, the upper half mirrored
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0;
      for (int b = 0; b < k; ++b) s += Mm[r][b] * Mm[c][b];
      if (mode == 1) { Pi[r * k + c] = s; Pi[c * k + r] = s; }
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
  for (int e = t; e < k * k; e += NT) {            // U = V^T M into A (its diagonal has been read): row t has norm cos(theta_t)
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b < k; ++b) s += V[b][r] * Mm[b][c];
    A[r][c] = s;
  }
  __syncthreads();
  if (t < k) {
    // Small angles take the sine from the eigenvalue of S (a difference of exactly accumulated entries); large ones take the COSINE from ||U_t||^2, a
    // sum of squares with full relative accuracy -- 1 - lambda has lost it there, and f = theta / (sin cos) divides by that cosine.
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
    // f = theta / (sin cos) and h = f cos^2 = theta cos / sin, both -> 1 as theta -> 0
    fv[t] = sn > 0.0 ? th / (sn * cs) : (sn == 0.0 ? 1.0 : sn);
    hv[t] = sn > 0.0 ? th * cs / sn : (sn == 0.0 ? 1.0 : sn);
  }
  __syncthreads();
  if (t < k) ths[rank_desc(thr, k, t)] = thr[t];       // descending; ties by index (rank counting)
  __syncthreads();
  for (int e = t; e < k; e += NT) thetas[i * k + e] = ths[e];
  if (t == 0) {
    double s = 0.0;
    for (int e = 0; e < k; ++e) s += ths[e] * ths[e];
    costs[i] = s;
    dom[i] = ths[0] > FR_DOMAIN ? 1 : 0;
  }
  if (mode == 1) return;
  double* Fb = FMt + i * k * k;
  for (int e = t; e < k * k; e += NT) {            // (F M)[a][b] = sum_t V[a][t] f_t U[t][b], stored transposed: element e = b k + a
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int x = 0; x < k; ++x) s += V[a][x] * fv[x] * A[x][b];
    Fb[e] = s;
  }
  for (int e = t; e < k * k; e += NT) {            // H_i = V h V^T, the upper half mirrored
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0;
      for (int x = 0; x < k; ++x) s += V[r][x] * hv[x] * V[c][x];
      Pi[r * k + c] = s; Pi[c * k + r] = s;
    }
  }
}

// one workgroup: H = sum_i H_i in index order, the cost of the iterate into the history, the domain flag
__global__ __launch_bounds__(256) void fr_mean_head_kernel(const double* Ps, double* H, const double* costs, const int* dom, FrCtl* ctl, double* hist_cost,
                                                           int B, int k, long cap) {
  const int done = ctl->done;
  __syncthreads();
  if (done) return;
  const int t = threadIdx.x;
  for (int e = t; e < k * k; e += 256) {
    double s = 0.0;
    for (long i = 0; i < B; ++i) s += Ps[i * k * k + e];
    H[e] = s;
  }
  if (t == 0) {
    if (ctl->iters >= cap) { ctl->done = 3; return; }
    double s = 0.0;
    for (int i = 0; i < B; ++i) s += costs[i];
    const double cost = 0.5 * s / B;
    hist_cost[ctl->iters] = cost;
    ctl->cost = cost;
    for (int i = 0; i < B; ++i)
      if (dom[i]) { ctl->domain = i; ctl->done = 2; break; }
  }
}

// rows of block i: C_T^T[r][a] = (FM^T[r][a] - sum_c H[a][c] C^T[r][c]) / B, in place on FMt
__global__ __launch_bounds__(256) void fr_tangent_kernel(double* CTt, const double* Ct, const double* H, const FrCtl* ctl, int B, int k) {
  if (ctl->done) return;
  const long base = (long)blockIdx.x * k * k;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int c = 0; c < k; ++c) s += H[a * k + c] * Ct[base + b * k + c];
    CTt[base + e] = (CTt[base + e] - s) / B;
  }
}

// Ps[i][a][c] = sum_b P^T[i k + b][a] Q^T[i k + b][c]: basis i's share of the k x k product P Q^T
__global__ __launch_bounds__(256) void fr_block_gram_kernel(const double* Pt, const double* Qt, double* Ps, const FrCtl* ctl, int k) {
  if (ctl->done) return;
  const long base = (long)blockIdx.x * k * k;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const int a = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b < k; ++b) s += Pt[base + b * k + a] * Qt[base + b * k + c];
    Ps[base + e] = s;
  }
}

// one workgroup: T T^T = sum_i Ps[i] = P Sigma^2 P^T, g = ||Sigma||_2 into the history, the convergence flag, and the two k x k factors of the exp map
// A1 = P cos(tau Sigma) P^T, A2 = P sin(tau Sigma) / Sigma P^T
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fr_step_head_kernel(const double* Ps, double* A1, double* A2, FrCtl* ctl, double* hist_g, int B, int k, double tau,
                                                          double tol) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], cs[KMAX], sn[KMAX], s2[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  __shared__ int conv;
  const int done = ctl->done;
  __syncthreads();
  if (done) return;
  const int t = threadIdx.x;
  for (int e = t; e < k * k; e += NT) {
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0;
      for (long i = 0; i < B; ++i) s += Ps[i * k * k + e];
      A[r][c] = s; A[c][r] = s;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(A, V, ws, k);
  if (t < k) {
    const double l = A[t][t];
    s2[t] = l < 0.0 ? 0.0 : l;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int e = 0; e < k; ++e) s += s2[e];
    const double g = sqrt(s);
    hist_g[ctl->iters] = g;
    ctl->g = g;
    conv = g < tol ? 1 : 0;
    if (conv) ctl->done = 1;
  }
  __syncthreads();
  if (conv) return;
  if (t < k) {
    const double sg = sqrt(s2[t]), x = tau * sg;
    cs[t] = cos(x);
    sn[t] = sg > 1e-8 ? sin(x) / sg : tau * (1.0 - x * x / 6.0);
  }
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {
    const int r = e / k, c = e % k;
    if (r <= c) {
      double p = 0.0, q = 0.0;
      for (int x = 0; x < k; ++x) { const double vv = V[r][x] * V[c][x]; p += vv * cs[x]; q += vv * sn[x]; }
      A1[r * k + c] = p; A1[c * k + r] = p;
      A2[r * k + c] = q; A2[c * k + r] = q;
    }
  }
}

// rows of block i of the exp map's image and of its product with Ghat: Cn^T = C^T A1^T + C_T^T A2^T, Nn^T = M^T A1^T + MT^T A2^T
__global__ __launch_bounds__(256) void fr_update_kernel(const double* Ct, const double* CTt, const double* Mt, const double* MTt, const double* A1,
                                                        const double* A2, double* Cn, double* Nn, const FrCtl* ctl, int k) {
  if (ctl->done) return;
  const long base = (long)blockIdx.x * k * k;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const int b = e / k, a = e % k;
    double s = 0.0, u = 0.0;
    for (int c = 0; c < k; ++c) {
      const double a1 = A1[a * k + c], a2 = A2[a * k + c];
      s += a1 * Ct[base + b * k + c] + a2 * CTt[base + b * k + c];
      u += a1 * Mt[base + b * k + c] + a2 * MTt[base + b * k + c];
    }
    Cn[base + e] = s;
    Nn[base + e] = u;
  }
}

// one workgroup: Gs = sum_i Ps[i] in index order (the Gram of the exp map's image; the whitening kernel mirrors its upper half)
__global__ __launch_bounds__(256) void fr_sum_kernel(const double* Ps, double* Gs, const FrCtl* ctl, int B, int k) {
  if (ctl->done) return;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    double s = 0.0;
    for (long i = 0; i < B; ++i) s += Ps[i * k * k + e];
    Gs[e] = s;
  }
}

// rows of block i: C^T[r][a] = sum_{b <= a} Wn[a][b] Cn^T[r][b] (Wn: the whitening of Gs, lower triangular); workgroup 0 counts the step
__global__ __launch_bounds__(256) void fr_apply_kernel(double* Ct, const double* Cn, const double* Wn, const int* bad, FrCtl* ctl, int k) {
  if (ctl->done) return;
  const long base = (long)blockIdx.x * k * k;
  const int nb = *bad;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int c = 0; c <= a; ++c) s += Wn[a * k + c] * Cn[base + b * k + c];
    Ct[base + e] = nb ? nan64() : s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->iters += 1; if (nb) ctl->reorth_bad = 1; }
}

// ------------------------------------------------------------------------------------------------------------ finish
// one workgroup: (1/B) sum_i M_i M_i^T = V diag(weight) V^T, descending; Rot[a][c] = V[c][order(a)]; theta [B][k] fp32; the final cost; info
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fr_finish_head_kernel(const double* Ps, const double* thetas, const double* costs, const int* flags, FrCtl* ctl,
                                                            double* hist_cost, const double* hist_g, double* Rot, float* weight, float* theta, double* info,
                                                            int B, int k, long cap) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], lam[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  const int t = threadIdx.x;
  for (int e = t; e < k * k; e += NT) {
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0;
      for (long i = 0; i < B; ++i) s += Ps[i * k * k + e];
      s /= B;
      A[r][c] = s; A[c][r] = s;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(A, V, ws, k);
  if (t < k) lam[t] = A[t][t];
  __syncthreads();
  if (t < k) {
    const int rank = rank_desc(lam, k, t);
    weight[rank] = (float)lam[t];
    for (int c = 0; c < k; ++c) Rot[rank * k + c] = V[c][t];
  }
  for (long e = t; e < (long)B * k; e += NT) theta[e] = (float)thetas[e];
  const int it = ctl->iters;
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < B; ++i) s += costs[i];
    const double cost = 0.5 * s / B;
    if (it <= cap) hist_cost[it] = cost;
    ctl->cost = cost;
    info[0] = (double)it; info[1] = ctl->g; info[2] = (double)ctl->done; info[3] = (double)ctl->domain; info[4] = (double)(it + 1);
    info[5] = (double)ctl->reorth_bad; info[6] = 0.0; info[7] = 0.0;
  }
  __syncthreads();
  double* ic = info + 8;
  double* ig = ic + cap + 1;
  double* ifl = ig + cap;
  for (long e = t; e <= cap; e += NT) ic[e] = e <= it ? hist_cost[e] : 0.0;
  for (long e = t; e < cap; e += NT) ig[e] = e < it || (e == it && ctl->done == 1) ? hist_g[e] : 0.0;
  for (long e = t; e < B; e += NT) ifl[e] = (double)flags[e];
}

// rows of block i of Z^T, Z = (Rot C) blockdiag(W): the coefficients of the mean's canonical basis on the rows of X as given
template <int KMAX>
__global__ __launch_bounds__(256) void fr_finish_coef_kernel(const double* Ct, const double* Rot, const double* W, const int* flags, double* Zt, int k) {
  __shared__ double Cp[KMAX][KMAX + 1];            // Cp[a][b] = (Rot C)[a][i k + b]
  const long base = (long)blockIdx.x * k * k;
  const int t = threadIdx.x;
  for (int e = t; e < k * k; e += 256) {
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int c = 0; c < k; ++c) s += Rot[a * k + c] * Ct[base + b * k + c];
    Cp[a][b] = s;
  }
  __syncthreads();
  const double* Wi = W + base;
  const int bad = flags[blockIdx.x];
  for (int e = t; e < k * k; e += 256) {
    const int b = e / k, a = e % k;
    double s = 0.0;
    for (int c = b; c < k; ++c) s += Cp[a][c] * Wi[c * k + b];
    Zt[base + e] = bad ? nan64() : s;
  }
}

// Y [k][N] fp32 = Z [k][R] X [R][N], one pass over X.  A wave owns 64 columns: lane (j = l & 15, g = l >> 4) loads the four columns 4j .. 4j+3 of row r0 + g
// in one 16-byte access and feeds column e to the MFMAs of tile e, so tile e holds the columns {4j + e}; the rows of X are summed in index order, four per
// MFMA, in fp64; one rounding at the store.  vec: 16-byte accesses are legal (N % 4 == 0, X and Y 16-byte aligned).
template <int KT>
__global__ __launch_bounds__(256) void fr_stream_kernel(const float* X, const double* Zt, float* Y, int R, int k, long N, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const long n0 = ((long)blockIdx.x * 4 + wave) * 64 + 4 * j;       // this lane's first column
  if (((long)blockIdx.x * 4 + wave) * 64 >= N) return;               // wave-uniform (no workgroup barrier in this kernel)
  geom_d4 acc[KT][4];
#pragma unroll
  for (int m = 0; m < KT; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[m][e] = geom_d4{0.0, 0.0, 0.0, 0.0};
  for (int r0 = 0; r0 < R; r0 += 4) {
    const int r = r0 + g;
    const float4 x = r < R ? load4(X + (long)r * N, n0, N, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
    mfma_rows4<KT>(acc, Zt, r, r < R, j, k, x);
  }
  if (n0 >= N) return;
#pragma unroll
  for (int m = 0; m < KT; ++m)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int a = 16 * m + g + 4 * x;
      if (a >= k) continue;
      store4(Y + (long)a * N, n0, N, vec, make_float4((float)acc[m][0][x], (float)acc[m][1][x], (float)acc[m][2][x], (float)acc[m][3][x]));
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
constexpr long FR_MAX_BASES = 65535;       // a grid axis of the whitening launch
constexpr long FR_MAX_ROWS = 1 << 20;      // R = B k (R^2 doubles must fit the scratch anyway)
constexpr long FR_MAX_ITER = 1 << 24;

namespace {
struct FrLayout {
  size_t ctl = 0, G = 0, W = 0, flags = 0, Ct = 0, CTt = 0, Mt = 0, MTt = 0, Cn = 0, Nn = 0, Ps = 0, small = 0, thetas = 0, costs = 0, hist = 0, total = 0;
};
bool fr_layout(long B, int k, long N, long cap, FrLayout& l) {
  if (B < 1 || B > FR_MAX_BASES || k < 1 || k > FRECHET_MAX_RANK || N < 1 || k > N || B * k > FR_MAX_ROWS || cap < 0 || cap > FR_MAX_ITER) return false;
  ScratchCarver s;
  const size_t R = (size_t)B * k, kk = (size_t)k * k * sizeof(double), rk = R * k * sizeof(double);
  l.ctl = s.take(sizeof(FrCtl));
  l.G = s.take(R * R * sizeof(double));
  l.W = s.take((size_t)B * kk);
  l.flags = s.take((2 * (size_t)B + 1) * sizeof(int));      // degenerate [B], domain [B], the re-orthonormalisation's flag
  l.Ct = s.take(rk); l.CTt = s.take(rk); l.Mt = s.take(rk); l.MTt = s.take(rk); l.Cn = s.take(rk); l.Nn = s.take(rk);
  l.Ps = s.take((size_t)B * kk);
  l.small = s.take(5 * kk);                                  // H, A1, A2, Gs, Rot
  l.thetas = s.take(R * sizeof(double));
  l.costs = s.take((size_t)B * sizeof(double));
  l.hist = s.take((2 * (size_t)cap + 1) * sizeof(double));   // cost [cap + 1], g [cap]
  l.total = s.off;
  return true;
}
struct FrPtrs {
  FrCtl* ctl; double *G, *W, *Ct, *CTt, *Mt, *MTt, *Cn, *Nn, *Ps, *H, *A1, *A2, *Gs, *Rot, *thetas, *costs, *hist_cost, *hist_g; int *flags, *dom, *rbad;
};
FrPtrs fr_ptrs(void* scratch, const FrLayout& l, long B, int k, long cap) {
  char* b = (char*)scratch;
  FrPtrs p;
  const size_t kk = (size_t)k * k;
  p.ctl = (FrCtl*)(b + l.ctl); p.G = (double*)(b + l.G); p.W = (double*)(b + l.W);
  p.flags = (int*)(b + l.flags); p.dom = p.flags + B; p.rbad = p.dom + B;
  p.Ct = (double*)(b + l.Ct); p.CTt = (double*)(b + l.CTt); p.Mt = (double*)(b + l.Mt); p.MTt = (double*)(b + l.MTt);
  p.Cn = (double*)(b + l.Cn); p.Nn = (double*)(b + l.Nn); p.Ps = (double*)(b + l.Ps);
  p.H = (double*)(b + l.small); p.A1 = p.H + kk; p.A2 = p.A1 + kk; p.Gs = p.A2 + kk; p.Rot = p.Gs + kk;
  p.thetas = (double*)(b + l.thetas); p.costs = (double*)(b + l.costs);
  p.hist_cost = (double*)(b + l.hist); p.hist_g = p.hist_cost + cap + 1;
  return p;
}
int fr_check(const char* who, long B, int k, long N, long cap, const void* scratch, size_t scratch_bytes, FrLayout& l) {
  if (!fr_layout(B, k, N, cap, l)) {
    set_error("%s: B=%ld outside [1,%ld], k=%d outside [1,%d], N=%ld < k, B k above %ld, or max_iter=%ld outside [0,%ld]", who, B, FR_MAX_BASES, k,
              FRECHET_MAX_RANK, N, FR_MAX_ROWS, cap, FR_MAX_ITER);
    return -1;
  }
  return check_scratch(who, scratch, scratch_bytes, l.total, "dpb_frechet_scratch_bytes(%ld, %d, %ld, %ld)", B, k, N, cap);
}

void fr_product(const FrPtrs& p, const double* In, double* Out, int R, int k, int force, hipStream_t st) {
  const dim3 grid((R + 15) / 16);
  DPB_BY_TILES(k, DPB_LAUNCH((fr_product_kernel<KT>), grid, dim3(256), 0, st, p.G, In, Out, R, k, p.ctl, force));
}
}  // namespace

// Ghat [R][R] of X [B][k][N] with its whitenings W [B][k][k] and degenerate flags [B]: the exact cross-Gram, each basis's own block whitened as
// angles.hip does, every block W_i G_ij W_j^T (shared with flagmean.hip)
int launch_whitened_gram(const float* X, long B, int k, long N, double* G, double* W, int* flags, hipStream_t st) {
  const int R = (int)(B * k);
  if (launch_cross_gram(X, nullptr, G, R, R, N, st) != 0) return -1;
  launch_gram_blocks(G, W, (int)B, R, k, k, st);                          // each basis's diagonal block of G into the slot its whitening matrix will take
  launch_angles_prep(W, flags, (int)B, k, st);
  const dim3 wg((unsigned)B, (unsigned)B);
  DPB_BY_RANK(k, (void)NT; DPB_LAUNCH((fr_whiten_kernel<KM>), wg, dim3(256), 0, st, G, W, flags, R, k));
  return 0;
}

// Y [k][N] fp32 = Z [k][R] X [R][N] with Z kept transposed (Zt [R][k]), k <= 64: fr_stream_kernel (shared with flagmean.hip)
int launch_coef_stream(const float* X, const double* Zt, float* Y, int R, int k, long N, hipStream_t st) {
  const int vec = (N % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0) ? 1 : 0;
  const dim3 sg((unsigned)((N + 255) / 256));
  DPB_BY_TILES(k, DPB_LAUNCH((fr_stream_kernel<KT>), sg, dim3(256), 0, st, X, Zt, Y, R, k, N, vec));
  return 0;
}

size_t frechet_scratch_bytes(long B, int k, long N, long max_iter) {
  FrLayout l;
  return fr_layout(B, k, N, max_iter, l) ? l.total : 0;
}

int launch_frechet_init(const float* X, long B, int k, long N, long max_iter, int init, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FrLayout l;
  if (fr_check("dpb_frechet_init", B, k, N, max_iter, scratch, scratch_bytes, l) != 0) return -1;
  if (init < 0 || init >= B) { set_error("dpb_frechet_init: init=%d outside [0,%ld)", init, B); return -1; }
  const FrPtrs p = fr_ptrs(scratch, l, B, k, max_iter);
  const int R = (int)(B * k);
  if (launch_whitened_gram(X, B, k, N, p.G, p.W, p.flags, st) != 0) return -1;
  DPB_LAUNCH(fr_init_kernel, dim3((unsigned)(((long)R * k + 255) / 256)), dim3(256), 0, st, p.Ct, p.ctl, R, k, init);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_frechet_iterate(long B, int k, long N, long max_iter, int n_iter, double step, double tol, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FrLayout l;
  if (fr_check("dpb_frechet_iterate", B, k, N, max_iter, scratch, scratch_bytes, l) != 0) return -1;
  if (n_iter < 0 || !(step > 0.0) || !(tol >= 0.0)) { set_error("dpb_frechet_iterate: n_iter=%d < 0, step=%g <= 0 or tol=%g < 0", n_iter, step, tol); return -1; }
  const FrPtrs p = fr_ptrs(scratch, l, B, k, max_iter);
  const int R = (int)(B * k), nb = (int)B;
  const dim3 gb((unsigned)B), one(1), t256(256);
  for (int it = 0; it < n_iter; ++it) {
    fr_product(p, p.Ct, p.Mt, R, k, 0, st);                                                                   // M = C Ghat
    DPB_BY_RANK(k, DPB_LAUNCH((fr_basis_kernel<KM, NT>), gb, dim3(NT), 0, st, p.Mt, p.CTt, p.Ps, p.thetas, p.costs, p.dom, p.ctl, k, 0));
    DPB_LAUNCH(fr_mean_head_kernel, one, t256, 0, st, p.Ps, p.H, p.costs, p.dom, p.ctl, p.hist_cost, nb, k, max_iter);
    DPB_LAUNCH(fr_tangent_kernel, gb, t256, 0, st, p.CTt, p.Ct, p.H, p.ctl, nb, k);                           // the mean tangent's coefficients
    fr_product(p, p.CTt, p.MTt, R, k, 0, st);                                                                 // C_T Ghat
    DPB_LAUNCH(fr_block_gram_kernel, gb, t256, 0, st, p.MTt, p.CTt, p.Ps, p.ctl, k);
    DPB_BY_RANK(k, DPB_LAUNCH((fr_step_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.Ps, p.A1, p.A2, p.ctl, p.hist_g, nb, k, step, tol));
    DPB_LAUNCH(fr_update_kernel, gb, t256, 0, st, p.Ct, p.CTt, p.Mt, p.MTt, p.A1, p.A2, p.Cn, p.Nn, p.ctl, k);   // the exp map
    DPB_LAUNCH(fr_block_gram_kernel, gb, t256, 0, st, p.Nn, p.Cn, p.Ps, p.ctl, k);
    DPB_LAUNCH(fr_sum_kernel, one, t256, 0, st, p.Ps, p.Gs, p.ctl, nb, k);
    launch_angles_prep(p.Gs, p.rbad, 1, k, st);                                                               // Gs -> its whitening, in place
    DPB_LAUNCH(fr_apply_kernel, gb, t256, 0, st, p.Ct, p.Cn, p.Gs, p.rbad, p.ctl, k);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_frechet_finish(const float* X, long B, int k, long N, long max_iter, float* Y, float* weight, float* theta, double* info, void* scratch,
                          size_t scratch_bytes, hipStream_t st) {
  FrLayout l;
  if (fr_check("dpb_frechet_finish", B, k, N, max_iter, scratch, scratch_bytes, l) != 0) return -1;
  const FrPtrs p = fr_ptrs(scratch, l, B, k, max_iter);
  const int R = (int)(B * k), nb = (int)B;
  const dim3 gb((unsigned)B), one(1), t256(256);
  fr_product(p, p.Ct, p.Mt, R, k, 1, st);
  DPB_BY_RANK(k, DPB_LAUNCH((fr_basis_kernel<KM, NT>), gb, dim3(NT), 0, st, p.Mt, p.CTt, p.Ps, p.thetas, p.costs, p.dom, p.ctl, k, 1));
  DPB_BY_RANK(k, DPB_LAUNCH((fr_finish_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.Ps, p.thetas, p.costs, p.flags, p.ctl, p.hist_cost, p.hist_g, p.Rot,
                           weight, theta, info, nb, k, max_iter));
  DPB_BY_RANK(k, (void)NT; DPB_LAUNCH((fr_finish_coef_kernel<KM>), gb, t256, 0, st, p.Ct, p.Rot, p.W, p.flags, p.Cn, k));
  if (launch_coef_stream(X, p.Cn, Y, R, k, N, st) != 0) return -1;
  DPB_CHECK(hipGetLastError());
  return 0;
}

const double* frechet_ghat(long B, int k, long N, long max_iter, const void* scratch) {
  FrLayout l;
  return fr_layout(B, k, N, max_iter, l) ? (const double*)((const char*)scratch + l.G) : nullptr;
}

// the parts of a Frechet scratch block that pga.hip reads after dpb_frechet_finish: Ghat, the whitenings, the flags, the base point's coefficients, the rotation
bool frechet_view(long B, int k, long N, long max_iter, void* scratch, FrechetView& v) {
  FrLayout l;
  if (!scratch || !fr_layout(B, k, N, max_iter, l)) return false;
  const FrPtrs p = fr_ptrs(scratch, l, B, k, max_iter);
  v.G = p.G; v.W = p.W; v.Ct = p.Ct; v.Rot = p.Rot; v.flags = p.flags; v.total = l.total;
  return true;
}

// the iteration restarted at the caller's point: C^T = Ct [R][k] (any full-rank coefficients on the whitened rows), whitened by the step's own
// re-orthonormalisation -- the Cholesky factor of C Ghat C^T; the status cleared
int launch_frechet_start(const double* Ct, long B, int k, long N, long max_iter, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FrLayout l;
  if (fr_check("dpb_frechet_start", B, k, N, max_iter, scratch, scratch_bytes, l) != 0) return -1;
  const FrPtrs p = fr_ptrs(scratch, l, B, k, max_iter);
  const int R = (int)(B * k), nb = (int)B;
  const dim3 gb((unsigned)B), one(1), t256(256);
  DPB_LAUNCH(fr_start_kernel, dim3((unsigned)(((long)R * k + 255) / 256)), t256, 0, st, Ct, p.Cn, p.ctl, (long)R * k, 0);
  fr_product(p, p.Cn, p.Nn, R, k, 1, st);
  DPB_LAUNCH(fr_block_gram_kernel, gb, t256, 0, st, p.Nn, p.Cn, p.Ps, p.ctl, k);
  DPB_LAUNCH(fr_sum_kernel, one, t256, 0, st, p.Ps, p.Gs, p.ctl, nb, k);
  launch_angles_prep(p.Gs, p.rbad, 1, k, st);
  DPB_LAUNCH(fr_apply_kernel, gb, t256, 0, st, p.Ct, p.Cn, p.Gs, p.rbad, p.ctl, k);
  DPB_LAUNCH(fr_start_kernel, one, t256, 0, st, Ct, p.Cn, p.ctl, 0L, 1);      // (the apply counted a step: none was taken)
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
