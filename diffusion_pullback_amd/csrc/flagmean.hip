// Flag (extrinsic, chordal) mean of B local bases of k rows in R^N (Draper et al. 2014; Marrinan et al., CVPR 2014): the top-r eigenvectors of the mean
// projector P = (1/B) sum_i Q_i^T Q_i, Q_i = W_i X_i the orthonormalised bases.  X [B][k][N] fp32, rows need not be orthonormal; R = B k.
//
// Every eigenvector with a non-zero eigenvalue lies in the span of the R rows, Y = C Q with C [r][R], and P (Q^T c) = (1/B) Q^T (Ghat c) with
// Ghat = Q Q^T [R][R] the whitened Gram dpb_frechet_init forms: the rows of C are the top eigenvectors z_j of Ghat scaled by 1 / sqrt(lambda_j), and
// weight_j = lambda_j / B.  The solver keeps Z [R][m], m >= r columns orthonormal in R^R, and per iteration
//   W = Ghat Z (the one pass over Ghat);  T = Z^T W = S Lambda S^T (Jacobi, descending);  res = max_{j<r} ||(W S)_j - lambda_j (Z S)_j||_2 / lambda_0;
//   Z <- orth(W S): through the eigen-decomposition of the Gram of W S, twice -- the first pass W S V D^-1/2 leaves an orthogonality error of
//   eps cond(W)^2, the second, symmetric one (Z1 (Z1^T Z1)^-1/2) removes it; columns whose D falls below 1e-13 D_max are dropped (set to zero: Ghat is
//   rank deficient when R > N or members share directions exactly), which keeps cond(W)^2 eps below 1e-3 for the second pass.
// finish takes the Rayleigh-Ritz step of the block as it stands in the ambient space (the pencil (W^T W, T)), so the rows returned are orthonormal and
// the values returned their Rayleigh quotients under the mean projector, converged or not; at convergence C = Lambda^-1/2 (Z S)^T.  Coefficient matrices are kept TRANSPOSED, [R][m], as frechet.hip keeps them.
// Reproducibility: fp64, no atomics, every sum a fixed chain -- the reduction range of the product is cut among the waves of a workgroup at bounds
// that depend on R only and the partial tiles are added in wave order; sums over rows run in chunks of 64 rows, the chunks added in index order.
#include "kernels.h"
#include "geom.h"

namespace dpb {

struct FmCtl {            // the first bytes of the scratch block (documented in dpb.h: the caller may read them)
  int done;               // 0 running, 1 converged (res <= tol), 2 a NaN met (a degenerate basis), 3 max_iter reached
  int iters;              // iterations taken
  int pad0, pad1;
  double res, lam0;       // the last residual computed; the largest Ritz value of that iteration
};

constexpr int FM_CHUNK = 64;           // rows per partial sum of the tall-skinny small algebra (one workgroup each: R / 64 of them fill the card at R = 5000)
constexpr int FM_TILE = 32;            // rows staged in LDS at a time
constexpr double FM_DROP = 1e-13;      // a direction of the block whose squared norm falls below this share of the largest is dropped

// the start block: a fixed function of (seed, element index), uniform in [-1, 1) (splitmix64)
__device__ inline double fm_start_value(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = (seed + 1ULL) * 0x9E3779B97F4A7C15ULL + idx * 0xD1B54A32D192ED03ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return (double)(long long)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

// Z = the identity (m == R: one Rayleigh-Ritz step is then exact) or the start block; the control block cleared
__global__ __launch_bounds__(256) void fm_init_kernel(double* Z, FmCtl* ctl, int R, int m, unsigned long long seed) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < (long)R * m) Z[e] = (m == R) ? ((e / m == e % m) ? 1.0 : 0.0) : fm_start_value(seed, (unsigned long long)e);
  if (e == 0) { ctl->done = 0; ctl->iters = 0; ctl->pad0 = 0; ctl->pad1 = 0; ctl->res = 0.0; ctl->lam0 = 0.0; }
}

// ------------------------------------------------------------------------------------------------------------ the skinny product with Ghat
// Out [R][m] = Ghat [R][R] Z [R][m] on v_mfma_f64_16x16x4_f64.  A workgroup owns 32 ROWS of Ghat (two 16-row tiles); its NW waves take an NW-th of the
// reduction range each, in chunks of 16 columns, and their partial tiles are added in wave order.  NW = 8: at R = 5000 the grid is 157 workgroups on
// 256 compute units, and the kernel lives on loads in flight; 4 is kept as the A/B switch DPB_FM_WAVES=4 (the cut points, and so the last bits, differ).  Lane (j = l & 15, g = l >> 4) reads the four
// consecutive doubles Ghat[row j][16 c + 4 g ..+3] of each tile in one 32-byte access -- the 16 lanes g, e of a row cover one 128-byte line, a wave's
// access 16 full lines -- and feeds element e to MFMA e of the chunk, so the k slot g of MFMA e is column 16 c + 4 g + e; the B operand is
// Z[16 c + 4 g + e][16 n + j], read through L2 once per chunk and used for both row tiles.  The next chunk's operands are loaded before the current
// chunk's MFMAs issue (two register sets, loop unrolled by two).  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.
template <int KT>
struct FmOperands {
  double a[2][4];
  double b[4][KT];
};

template <int KT>
__device__ __forceinline__ void fm_load(FmOperands<KT>& o, const double* __restrict__ G, const double* __restrict__ Z, int c, int c_hi, int i0, int j, int g,
                                        int R, int m, bool vec) {
  const int col = 16 * c + 4 * g;
  const bool live = c < c_hi;
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const int row = i0 + 16 * tl + j;
    const bool ok = live && row < R && col < R;
    if (ok && vec) {
      const geom_d4 v = *reinterpret_cast<const geom_d4*>(G + (long)row * R + col);
      o.a[tl][0] = v[0]; o.a[tl][1] = v[1]; o.a[tl][2] = v[2]; o.a[tl][3] = v[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o.a[tl][e] = (ok && col + e < R) ? G[(long)row * R + col + e] : 0.0;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int zr = col + e;
#pragma unroll
    for (int n = 0; n < KT; ++n) o.b[e][n] = (live && zr < R && 16 * n + j < m) ? Z[(long)zr * m + 16 * n + j] : 0.0;
  }
}

template <int KT>
__device__ __forceinline__ void fm_mma(geom_d4 (&acc)[2][KT], const FmOperands<KT>& o) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int n = 0; n < KT; ++n) {
      acc[0][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[0][e], o.b[e][n], acc[0][n], 0, 0, 0);
      acc[1][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[1][e], o.b[e][n], acc[1][n], 0, 0, 0);
    }
}

template <int KT, int NW>
__global__ __launch_bounds__(NW * 64) void fm_product_kernel(const double* __restrict__ G, const double* __restrict__ Z, double* __restrict__ Out, int R, int m,
                                                         const FmCtl* ctl, int force) {
  if (!force && ctl->done) return;
  __shared__ double red[NW][2][KT][4][64];
  static_assert(sizeof(double) * NW * 2 * KT * 4 * 64 <= 160 * 1024, "fm_product_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * 32;
  const int chunks = (R + 15) / 16, q = (chunks + NW - 1) / NW;
  const int c_lo = wave * q, c_hi = c_lo + q < chunks ? c_lo + q : chunks;
  const bool vec = (R & 3) == 0;                      // every row of Ghat starts on a 32-byte boundary
  geom_d4 acc[2][KT];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int n = 0; n < KT; ++n) acc[tl][n] = geom_d4{0.0, 0.0, 0.0, 0.0};
  FmOperands<KT> o0, o1;
  fm_load<KT>(o0, G, Z, c_lo, c_hi, i0, j, g, R, m, vec);
  for (int c = c_lo; c < c_hi; c += 2) {               // (a chunk past c_hi loads zeros: its MFMAs add nothing)
    fm_load<KT>(o1, G, Z, c + 1, c_hi, i0, j, g, R, m, vec);
    fm_mma<KT>(acc, o0);
    fm_load<KT>(o0, G, Z, c + 2, c_hi, i0, j, g, R, m, vec);
    fm_mma<KT>(acc, o1);
  }
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int n = 0; n < KT; ++n)
#pragma unroll
      for (int x = 0; x < 4; ++x) red[wave][tl][n][x][lane] = acc[tl][n][x];
  __syncthreads();
  for (int e = t; e < 2 * KT * 4 * 64; e += NW * 64) {
    const int ln = e & 63, x = (e >> 6) & 3, n = (e >> 8) % KT, tl = (e >> 8) / KT;
    double v = red[0][tl][n][x][ln];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w][tl][n][x][ln];
    const int row = i0 + 16 * tl + (ln >> 4) + 4 * x, col = 16 * n + (ln & 15);
    if (row < R && col < m) Out[(long)row * m + col] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------ the tall-skinny small algebra
// chunk ch of 64 rows: part[ch][0] = A_ch^T B_ch and, with both, part[ch][1] = B_ch^T B_ch ([m][m] each); rows in index order
__global__ __launch_bounds__(256) void fm_gram_kernel(const double* A, const double* Bm, double* part, int R, int m, int both, const FmCtl* ctl, int force) {
  if (!force && ctl->done) return;
  __shared__ double At[FM_TILE][65], Bt[FM_TILE][65];
  const int t = threadIdx.x, mm = m * m;
  const long r_lo = (long)blockIdx.x * FM_CHUNK;
  const long r_hi = r_lo + FM_CHUNK < R ? r_lo + FM_CHUNK : R;
  double s1[16], s2[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { s1[i] = 0.0; s2[i] = 0.0; }
  for (long r0 = r_lo; r0 < r_hi; r0 += FM_TILE) {
    for (int e = t; e < FM_TILE * m; e += 256) {
      const int rr = e / m, c = e % m;
      const bool ok = r0 + rr < r_hi;
      At[rr][c] = ok ? A[(r0 + rr) * m + c] : 0.0;
      Bt[rr][c] = ok ? Bm[(r0 + rr) * m + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = t + 256 * i;
      if (e < mm) {
        const int a = e / m, b = e % m;
        double u = s1[i], v = s2[i];
        for (int rr = 0; rr < FM_TILE; ++rr) {
          u += At[rr][a] * Bt[rr][b];
          if (both) v += Bt[rr][a] * Bt[rr][b];
        }
        s1[i] = u; s2[i] = v;
      }
    }
    __syncthreads();
  }
  double* p = part + (long)blockIdx.x * 2 * mm;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = t + 256 * i;
    if (e < mm) { p[e] = s1[i]; if (both) p[mm + e] = s2[i]; }
  }
}

// Out [R][nc] = In [R][m] Mx[:, :nc] (Mx [m][m] row-major), rows in tiles of 32
__global__ __launch_bounds__(256) void fm_rowmul_kernel(const double* In, const double* Mx, double* Out, int R, int m, int nc, const FmCtl* ctl, int force) {
  if (!force && ctl->done) return;
  __shared__ double Ml[64][65], It[FM_TILE][65];
  const int t = threadIdx.x;
  for (int e = t; e < m * m; e += 256) Ml[e / m][e % m] = Mx[e];
  const long r_lo = (long)blockIdx.x * FM_CHUNK;
  const long r_hi = r_lo + FM_CHUNK < R ? r_lo + FM_CHUNK : R;
  for (long r0 = r_lo; r0 < r_hi; r0 += FM_TILE) {
    __syncthreads();
    for (int e = t; e < FM_TILE * m; e += 256) {
      const int rr = e / m, c = e % m;
      It[rr][c] = r0 + rr < r_hi ? In[(r0 + rr) * m + c] : 0.0;
    }
    __syncthreads();
    for (int e = t; e < FM_TILE * nc; e += 256) {
      const int rr = e / nc, c = e % nc;
      if (r0 + rr >= r_hi) continue;
      double s = 0.0;
      for (int b = 0; b < m; ++b) s += It[rr][b] * Ml[b][c];
      Out[(r0 + rr) * nc + c] = s;
    }
  }
}

// the move of an iteration and its residual: Z1 = W A (A = S V D^-1/2 of the head), and per column j the chunk's share of
// ||(W S)_j - lambda_j (Z S)_j||^2 into respart[ch][j]
__global__ __launch_bounds__(256) void fm_move_kernel(const double* Z, const double* Wb, const double* S, const double* Amat, const double* lam, double* Z1,
                                                      double* respart, int R, int m, const FmCtl* ctl) {
  if (ctl->done) return;
  __shared__ double Sl[64][65], Al[64][65], Wt[FM_TILE][65], Zt[FM_TILE][65], Dt[FM_TILE][65];
  static_assert(sizeof(double) * 65 * (2 * 64 + 3 * FM_TILE) <= 160 * 1024, "fm_move_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  for (int e = t; e < m * m; e += 256) { Sl[e / m][e % m] = S[e]; Al[e / m][e % m] = Amat[e]; }
  const long r_lo = (long)blockIdx.x * FM_CHUNK;
  const long r_hi = r_lo + FM_CHUNK < R ? r_lo + FM_CHUNK : R;
  double racc = 0.0;
  for (long r0 = r_lo; r0 < r_hi; r0 += FM_TILE) {
    __syncthreads();
    for (int e = t; e < FM_TILE * m; e += 256) {
      const int rr = e / m, c = e % m;
      const bool ok = r0 + rr < r_hi;
      Wt[rr][c] = ok ? Wb[(r0 + rr) * m + c] : 0.0;
      Zt[rr][c] = ok ? Z[(r0 + rr) * m + c] : 0.0;
    }
    __syncthreads();
    for (int e = t; e < FM_TILE * m; e += 256) {
      const int rr = e / m, c = e % m;
      double p = 0.0, qz = 0.0, z1 = 0.0;
      for (int b = 0; b < m; ++b) {
        const double w = Wt[rr][b], s = Sl[b][c];
        p += w * s; qz += Zt[rr][b] * s; z1 += w * Al[b][c];
      }
      const double d = p - lam[c] * qz;
      Dt[rr][c] = d * d;                             // (a row past the chunk is all zeros: d = 0)
      if (r0 + rr < r_hi) Z1[(r0 + rr) * m + c] = z1;
    }
    __syncthreads();
    if (t < m)
      for (int rr = 0; rr < FM_TILE; ++rr) racc += Dt[rr][t];
  }
  if (t < m) respart[(long)blockIdx.x * m + t] = racc;
}

// the sum of nch partial [m][m] matrices (stride pstride doubles) in chunk order into the LDS matrix A, the upper half mirrored; returns (uniformly)
// whether a NaN was met
template <int KMAX, int NT>
__device__ __forceinline__ bool fm_sum_parts(double (*A)[KMAX + 1], const double* part, long pstride, int nch, int m, double* red) {
  double bad = 0.0;
  for (int e = threadIdx.x; e < m * m; e += NT) {
    const int r = e / m, c = e % m;
    if (r <= c) {
      double s = 0.0;
      for (long ch = 0; ch < nch; ++ch) s += part[ch * pstride + e];
      A[r][c] = s; A[c][r] = s;
      if (s != s) bad = 1.0;
    }
  }
  return block_sum<NT>(bad, red) != 0.0;               // (block_sum's barriers also order the stores to A)
}

// one workgroup, the Rayleigh-Ritz step: T = sum of the partial Z^T W = S Lambda S^T, descending; the Gram of W S, S^T (W^T W) S = V D V^T; A = S V D+^-1/2.
// S, lam and A to global; max_iter reached: done = 3; a NaN: done = 2
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fm_head_kernel(const double* part, double* S, double* lam, double* Amat, FmCtl* ctl, int nch, int m, long max_iter) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], Nm[KMAX][KMAX + 1], lv[KMAX], dinv[KMAX], red[NT / 64];
  __shared__ int rk[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (3 * KMAX * (KMAX + 1) + 3 * KMAX + 16) + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "fm_head_kernel exceeds the gfx950 LDS");
  const int done = ctl->done, iters = ctl->iters;
  __syncthreads();
  if (done) return;
  const int t = threadIdx.x;
  if (iters >= max_iter) { if (t == 0) ctl->done = 3; return; }
  const long mm = (long)m * m;
  const bool bad1 = fm_sum_parts<KMAX, NT>(A, part, 2 * mm, nch, m, red);
  const bool bad2 = fm_sum_parts<KMAX, NT>(Nm, part + mm, 2 * mm, nch, m, red);
  if (bad1 || bad2) { if (t == 0) { ctl->done = 2; ctl->res = nan64(); } return; }
  jacobi_lds<KMAX, NT>(A, V, ws, m);
  if (t < m) lv[t] = A[t][t];
  __syncthreads();
  if (t < m) { rk[t] = rank_desc(lv, m, t); lam[rk[t]] = lv[t]; }
  __syncthreads();
  if (t == 0) { double l0 = lv[0]; for (int e = 1; e < m; ++e) l0 = lv[e] > l0 ? lv[e] : l0; ctl->lam0 = l0; }
  for (int e = t; e < m * m; e += NT) {                // A <- S: the eigenvectors as columns, descending
    const int a = e / m, c = e % m;
    const double v = V[a][c];
    A[a][rk[c]] = v;
    S[a * m + rk[c]] = v;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += NT) {                // V <- (W^T W) S
    const int a = e / m, b = e % m;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s += Nm[a][c] * A[c][b];
    V[a][b] = s;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += NT) {                // Nm <- S^T (W^T W) S, the upper half mirrored
    const int a = e / m, b = e % m;
    if (a <= b) {
      double s = 0.0;
      for (int c = 0; c < m; ++c) s += A[c][a] * V[c][b];
      Nm[a][b] = s; Nm[b][a] = s;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(Nm, V, ws, m);
  if (t < m) lv[t] = Nm[t][t];
  __syncthreads();
  if (t < m) {
    double dmax = 0.0;
    for (int e = 0; e < m; ++e) dmax = lv[e] > dmax ? lv[e] : dmax;
    dinv[t] = (lv[t] > FM_DROP * dmax && lv[t] > 0.0) ? 1.0 / sqrt(lv[t]) : 0.0;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += NT) {
    const int a = e / m, b = e % m;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s += A[a][c] * V[c][b];
    Amat[e] = s * dinv[b];
  }
}

// one workgroup, the second orthonormalisation: the Gram of Z1 = V D V^T, A2 = V D+^-1/2 V^T to global.  mode 1 (an iteration): also the residual
// max_{j<r} sqrt(sum of respart[.][j]) / lam0, the step counted, done = 1 when it is <= tol (the block then does not move).  mode 0: the start block
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fm_orth_head_kernel(const double* part, const double* respart, double* Amat, FmCtl* ctl, int nch, int m, int r, double tol,
                                                          int mode) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], lv[KMAX], dinv[KMAX], rs[KMAX], red[NT / 64];
  __shared__ JacobiWs<KMAX> ws;
  const int done = ctl->done;
  __syncthreads();
  if (done) return;
  const int t = threadIdx.x;
  const long mm = (long)m * m;
  const bool bad = fm_sum_parts<KMAX, NT>(A, part, 2 * mm, nch, m, red);
  if (bad) { if (t == 0) { ctl->done = 2; ctl->res = nan64(); } return; }
  jacobi_lds<KMAX, NT>(A, V, ws, m);
  if (t < m) lv[t] = A[t][t];
  __syncthreads();
  if (t < m) {
    double dmax = 0.0;
    for (int e = 0; e < m; ++e) dmax = lv[e] > dmax ? lv[e] : dmax;
    dinv[t] = (lv[t] > FM_DROP * dmax && lv[t] > 0.0) ? 1.0 / sqrt(lv[t]) : 0.0;
  }
  if (mode == 1 && t < r) {
    double s = 0.0;
    for (long ch = 0; ch < nch; ++ch) s += respart[ch * m + t];
    rs[t] = sqrt(s);
  }
  __syncthreads();
  for (int e = t; e < m * m; e += NT) {
    const int a = e / m, b = e % m;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s += V[a][c] * dinv[c] * V[b][c];
    Amat[e] = s;
  }
  if (mode == 1 && t == 0) {
    double worst = 0.0;
    bool isnan_ = false;
    for (int e = 0; e < r; ++e) { if (rs[e] != rs[e]) isnan_ = true; worst = rs[e] > worst ? rs[e] : worst; }
    const double res = isnan_ ? nan64() : (ctl->lam0 > 0.0 ? worst / ctl->lam0 : worst);
    ctl->res = res;
    ctl->iters += 1;
    if (isnan_) ctl->done = 2;
    else if (res <= tol) ctl->done = 1;
  }
}

// ------------------------------------------------------------------------------------------------------------ finish
// one workgroup: the Rayleigh-Ritz step of the block as it stands, in the AMBIENT space -- over the rows y = c^T Z^T Q the mean projector has
// y^T P y = c^T (W^T W) c / B and y^T y = c^T T c, so the pencil (W^T W, T) is solved: T = S Lambda S^T (Jacobi; directions below 1e-13 of the largest
// dropped), H = Lambda^-1/2 S^T (W^T W) S Lambda^-1/2 = U Mu U^T (Jacobi), descending.  Sc = S Lambda^-1/2 U [m][m]: C = Sc^T Z^T has C Ghat C^T = I whether
// the block has converged or not, and mu_j / B is the Rayleigh quotient of row j; at convergence mu = Lambda.  weight [r] fp32 = mu_j / B; info (dpb.h).
// A NaN: everything NaN
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fm_finish_head_kernel(const double* part, const double* G, double* Sc, float* weight, double* info, const FmCtl* ctl,
                                                            int nch, int m, int r, int B, int k, long R) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], Nm[KMAX][KMAX + 1], lv[KMAX], linv[KMAX], red[NT / 64];
  __shared__ int rk[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (3 * KMAX * (KMAX + 1) + 2 * KMAX + 16) + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "fm_finish_head_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  const long mm = (long)m * m;
  const bool bad1 = fm_sum_parts<KMAX, NT>(A, part, 2 * mm, nch, m, red);
  const bool bad2 = fm_sum_parts<KMAX, NT>(Nm, part + mm, 2 * mm, nch, m, red);
  const bool bad = bad1 || bad2;
  if (t == 0) {
    info[0] = (double)ctl->iters; info[1] = bad ? 2.0 : (double)ctl->done; info[2] = bad ? nan64() : ctl->res; info[3] = (double)m;
    info[4] = 0.0; info[5] = 0.0; info[6] = 0.0; info[7] = 0.0;
  }
  for (long e = t; e < B; e += NT) { const double d = G[(e * k) * (R + 1)]; info[8 + 64 + e] = d != d ? 1.0 : 0.0; }
  if (bad) {
    for (int e = t; e < m * m; e += NT) Sc[e] = nan64();
    for (int e = t; e < 64; e += NT) info[8 + e] = e < m ? nan64() : 0.0;
    for (int e = t; e < r; e += NT) weight[e] = (float)nan64();
    return;
  }
  jacobi_lds<KMAX, NT>(A, V, ws, m);
  if (t < m) lv[t] = A[t][t];
  __syncthreads();
  if (t < m) {
    double lmax = 0.0;
    for (int e = 0; e < m; ++e) lmax = lv[e] > lmax ? lv[e] : lmax;
    linv[t] = (lv[t] > FM_DROP * lmax && lv[t] > 0.0) ? 1.0 / sqrt(lv[t]) : 0.0;
  }
  for (int e = t; e < m * m; e += NT) {                // A <- (W^T W) S
    const int a = e / m, b = e % m;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s += Nm[a][c] * V[c][b];
    A[a][b] = s;
  }
  __syncthreads();
  for (int e = t; e < m * m; e += NT) {                // Nm <- H, the upper half mirrored
    const int a = e / m, b = e % m;
    if (a <= b) {
      double s = 0.0;
      for (int c = 0; c < m; ++c) s += V[c][a] * A[c][b];
      s *= linv[a] * linv[b];
      Nm[a][b] = s; Nm[b][a] = s;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(Nm, A, ws, m);                  // U into A
  if (t < m) lv[t] = Nm[t][t];
  __syncthreads();
  if (t < m) rk[t] = rank_desc(lv, m, t);
  for (int e = t; e < 64; e += NT) info[8 + e] = 0.0;
  __syncthreads();
  if (t < m) {
    info[8 + rk[t]] = lv[t];
    if (rk[t] < r) weight[rk[t]] = (float)(lv[t] / B);
  }
  for (int e = t; e < m * m; e += NT) {                // Sc = S Lambda^-1/2 U, the columns in descending order of mu
    const int a = e / m, b = e % m;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s += V[a][c] * linv[c] * A[c][b];
    Sc[a * m + rk[b]] = s;
  }
}

// one workgroup: sgn[j] = the sign of the entry of largest magnitude of column j of Ct [R][r] (the lowest row on a tie; +1 for a zero or NaN column)
__global__ __launch_bounds__(256) void fm_sign_kernel(const double* Ct, double* sgn, long R, int r) {
  __shared__ double bv[256], bs[256];
  __shared__ long bi[256];
  const int t = threadIdx.x;
  for (int j = 0; j < r; ++j) {
    double best = 0.0, sg = 1.0;
    long idx = 0;
    for (long row = t; row < R; row += 256) {
      const double v = Ct[row * r + j], a = fabs(v);
      if (a > best) { best = a; idx = row; sg = v < 0.0 ? -1.0 : 1.0; }
    }
    bv[t] = best; bi[t] = idx; bs[t] = sg;
    __syncthreads();
    if (t == 0) {
      double b = 0.0, s = 1.0;
      long ix = 0;
      for (int e = 0; e < 256; ++e)
        if (bv[e] > b || (bv[e] == b && b > 0.0 && bi[e] < ix)) { b = bv[e]; ix = bi[e]; s = bs[e]; }
      sgn[j] = s;
    }
    __syncthreads();
  }
}

// block i: the signs applied to Ct (the caller's [R][r]) and to Mt in place and, with W, the rows of Zc^T, Zc = C blockdiag(W): the coefficients of the
// mean's rows on the rows of X as given (a degenerate basis: NaN)
__global__ __launch_bounds__(256) void fm_coef_kernel(double* Ct, double* Mt, const double* sgn, const double* W, const double* G, double* Zc, int k, int r,
                                                      long R) {
  __shared__ double Cb[64][65];
  const long base = (long)blockIdx.x * k * r;
  const int t = threadIdx.x;
  for (int e = t; e < k * r; e += 256) {
    const int b = e / r, a = e % r;
    const double v = Ct[base + e] * sgn[a];
    Cb[b][a] = v;
    Ct[base + e] = v;
    Mt[base + e] *= sgn[a];
  }
  if (!W) return;
  __syncthreads();
  const double* Wi = W + (long)blockIdx.x * k * k;
  const double d = G[((long)blockIdx.x * k) * (R + 1)];
  const bool bad = d != d;
  for (int e = t; e < k * r; e += 256) {
    const int b = e / r, a = e % r;
    double s = 0.0;
    for (int c = b; c < k; ++c) s += Cb[c][a] * Wi[c * k + b];
    Zc[base + e] = bad ? nan64() : s;
  }
}

// One workgroup per basis i: theta [d] fp32, d = min(r, k), descending, from block i of Mt (M_i = Y Q_i^T, [r][k], stored [k][r]): on the smaller Gram
// shape I - Mm Mm^T = V sin^2(theta) V^T with Mm [d][D] = M_i or its transpose; small angles from the eigenvalue, large ones from the cosine
// ||(V^T Mm)_t||, as the log map of frechet.hip takes them
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void fm_theta_kernel(const double* Mt, float* theta, int k, int r) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], Mm[KMAX][KMAX + 1], lam[KMAX], thr[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (3 * KMAX * (KMAX + 1) + 2 * KMAX) + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "fm_theta_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  const long i = blockIdx.x;
  const double* Mb = Mt + i * k * r;
  const bool tr = r > k;                               // Mm = M_i^T [k][r]
  const int d = tr ? k : r, D = tr ? r : k;
  for (int e = t; e < k * r; e += NT) {
    const int b = e / r, a = e % r;                    // M_i[a][b]
    if (tr) Mm[b][a] = Mb[e]; else Mm[a][b] = Mb[e];
  }
  __syncthreads();
  for (int e = t; e < d * d; e += NT) {
    const int p = e / d, c = e % d;
    if (p <= c) {
      double s = 0.0;
      for (int b = 0; b < D; ++b) s += Mm[p][b] * Mm[c][b];
      const double v = (p == c ? 1.0 : 0.0) - s;
      A[p][c] = v; A[c][p] = v;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(A, V, ws, d);
  if (t < d) {
    const double l = A[t][t];
    lam[t] = l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);      // (a NaN stays a NaN)
  }
  __syncthreads();
  if (t < d) {
    const double l = lam[t];
    double th;
    if (l <= 0.5) {
      th = asin(sqrt(l));
    } else {
      double c2 = 0.0;
      for (int b = 0; b < D; ++b) {
        double u = 0.0;
        for (int a = 0; a < d; ++a) u += V[a][t] * Mm[a][b];
        c2 += u * u;
      }
      c2 = c2 > 1.0 ? 1.0 : c2;
      th = acos(sqrt(c2));
    }
    thr[t] = th;
  }
  __syncthreads();
  if (t < d) theta[i * d + rank_desc(thr, d, t)] = (float)thr[t];
}

// ------------------------------------------------------------------------------------------------------------ host side
namespace {
struct FmLayout {
  size_t ctl = 0, Z = 0, Wb = 0, Z1 = 0, part = 0, respart = 0, small = 0, W = 0, flags = 0, G = 0, total = 0;
  int m = 0, nch = 0;
};
// own: the block holds Ghat, the whitenings and the degenerate flags (at its end); otherwise the solver's part only
bool fm_layout(long B, int k, long N, int r, long max_iter, bool own, FmLayout& l) {
  if (B < 1 || B > 65535 || k < 1 || k > FRECHET_MAX_RANK || B * k > (1 << 20) || max_iter < 0 || max_iter > (1 << 24)) return false;
  const long R = B * k;
  if (r < 1 || r > FLAG_MEAN_MAX_RANK || r > R) return false;
  if (own && (N < 1 || k > N || r > N)) return false;       // (a caller's Ghat: its maker has checked N)
  l.m = flag_mean_block_width(R, r);
  l.nch = (int)((R + FM_CHUNK - 1) / FM_CHUNK);
  ScratchCarver s;
  const size_t rm = (size_t)R * l.m * sizeof(double), mm = (size_t)l.m * l.m * sizeof(double);
  l.ctl = s.take(sizeof(FmCtl));
  l.Z = s.take(rm); l.Wb = s.take(rm); l.Z1 = s.take(rm);
  l.part = s.take((size_t)l.nch * 2 * mm);
  l.respart = s.take((size_t)l.nch * l.m * sizeof(double));
  l.small = s.take(2 * mm + 2 * 64 * sizeof(double));        // S, A, lam [64], sgn [64]
  if (own) {
    l.W = s.take((size_t)B * k * k * sizeof(double));
    l.flags = s.take((size_t)B * sizeof(int));
    l.G = s.take((size_t)R * R * sizeof(double));
  }
  l.total = s.off;
  return true;
}
struct FmPtrs {
  FmCtl* ctl; double *Z, *Wb, *Z1, *part, *respart, *S, *A, *lam, *sgn, *W; const double* G; int* flags;
};
FmPtrs fm_ptrs(void* scratch, const FmLayout& l, const double* ghat) {
  char* b = (char*)scratch;
  FmPtrs p;
  const size_t mm = (size_t)l.m * l.m;
  p.ctl = (FmCtl*)(b + l.ctl); p.Z = (double*)(b + l.Z); p.Wb = (double*)(b + l.Wb); p.Z1 = (double*)(b + l.Z1);
  p.part = (double*)(b + l.part); p.respart = (double*)(b + l.respart);
  p.S = (double*)(b + l.small); p.A = p.S + mm; p.lam = p.A + mm; p.sgn = p.lam + 64;
  p.W = ghat ? nullptr : (double*)(b + l.W);
  p.flags = ghat ? nullptr : (int*)(b + l.flags);
  p.G = ghat ? ghat : (const double*)(b + l.G);
  return p;
}
int fm_check(const char* who, long B, int k, long N, int r, long max_iter, const double* ghat, const void* scratch, size_t scratch_bytes, FmLayout& l) {
  if (!fm_layout(B, k, N, r, max_iter, ghat == nullptr, l)) {
    set_error("%s: B=%ld outside [1,65535], k=%d outside [1,%d], N=%ld < k, B k above 2^20, r=%d outside [1,min(%d,B k,N)] or max_iter=%ld outside [0,2^24]",
              who, B, k, FRECHET_MAX_RANK, N, r, FLAG_MEAN_MAX_RANK, max_iter);
    return -1;
  }
  if (ghat && (uintptr_t)ghat % 32) { set_error("%s: Ghat must be 32-byte aligned", who); return -1; }
  return ghat ? check_scratch(who, scratch, scratch_bytes, l.total, "dpb_flag_mean_solver_bytes(%ld, %d, %d, %ld)", B, k, r, max_iter)
              : check_scratch(who, scratch, scratch_bytes, l.total, "dpb_flag_mean_scratch_bytes(%ld, %d, %ld, %d, %ld)", B, k, N, r, max_iter);
}

const int g_fm_waves = getenv("DPB_FM_WAVES") && atoi(getenv("DPB_FM_WAVES")) == 4 ? 4 : 8;      // A/B switch of the product kernel's workgroup size

void fm_product(const FmPtrs& p, const FmLayout& l, int R, int force, hipStream_t st) {
  const dim3 grid((R + 31) / 32);
  if (g_fm_waves == 4) DPB_BY_TILES(l.m, DPB_LAUNCH((fm_product_kernel<KT, 4>), grid, dim3(256), 0, st, p.G, p.Z, p.Wb, R, l.m, p.ctl, force));
  else DPB_BY_TILES(l.m, DPB_LAUNCH((fm_product_kernel<KT, 8>), grid, dim3(512), 0, st, p.G, p.Z, p.Wb, R, l.m, p.ctl, force));
}
// In <- In (In^T In)^-1/2 into Out (the symmetric orthonormalisation; mode 0) -- or the second pass of an iteration (mode 1)
void fm_orth_pass(const FmPtrs& p, const FmLayout& l, const double* In, double* Out, int R, int r, double tol, int mode, hipStream_t st) {
  const dim3 gc(l.nch), one(1), t256(256);
  DPB_LAUNCH(fm_gram_kernel, gc, t256, 0, st, In, In, p.part, R, l.m, 0, p.ctl, 0);
  DPB_BY_RANK(l.m, DPB_LAUNCH((fm_orth_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.part, p.respart, p.A, p.ctl, l.nch, l.m, r, tol, mode));
  DPB_LAUNCH(fm_rowmul_kernel, gc, t256, 0, st, In, p.A, Out, R, l.m, l.m, p.ctl, 0);
}
}  // namespace

int flag_mean_block_width(long R, int r) {
  long m = (r + 8 + 15) / 16 * 16;                     // at least 8 columns of oversampling, a whole number of 16-column MFMA tiles
  if (m > 64) m = 64;
  if (m > R) m = R;
  return (int)m;
}

size_t flag_mean_scratch_bytes(long B, int k, long N, int r, long max_iter, bool own) {
  FmLayout l;
  return fm_layout(B, k, N, r, max_iter, own, l) ? l.total : 0;
}

int launch_flag_mean_init(const float* X, const double* ghat, long B, int k, long N, int r, unsigned long long seed, long max_iter, void* scratch,
                          size_t scratch_bytes, hipStream_t st) {
  FmLayout l;
  if (fm_check("dpb_flag_mean_init", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, l) != 0) return -1;
  const FmPtrs p = fm_ptrs(scratch, l, ghat);
  const int R = (int)(B * k);
  if (!ghat && launch_whitened_gram(X, B, k, N, (double*)p.G, p.W, p.flags, st) != 0) return -1;
  DPB_LAUNCH(fm_init_kernel, dim3((unsigned)(((long)R * l.m + 255) / 256)), dim3(256), 0, st, p.Z, p.ctl, R, l.m, seed);
  if (l.m != R) {                                      // the start block orthonormalised, twice
    fm_orth_pass(p, l, p.Z, p.Z1, R, r, 0.0, 0, st);
    fm_orth_pass(p, l, p.Z1, p.Z, R, r, 0.0, 0, st);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_mean_iterate(const double* ghat, long B, int k, long N, int r, long max_iter, int n_iter, double tol, void* scratch, size_t scratch_bytes,
                             hipStream_t st) {
  FmLayout l;
  if (fm_check("dpb_flag_mean_iterate", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, l) != 0) return -1;
  if (n_iter < 0 || !(tol >= 0.0)) { set_error("dpb_flag_mean_iterate: n_iter=%d < 0 or tol=%g < 0", n_iter, tol); return -1; }
  const FmPtrs p = fm_ptrs(scratch, l, ghat);
  const int R = (int)(B * k);
  const dim3 gc(l.nch), one(1), t256(256);
  for (int it = 0; it < n_iter; ++it) {
    fm_product(p, l, R, 0, st);                                                                                // W = Ghat Z
    DPB_LAUNCH(fm_gram_kernel, gc, t256, 0, st, p.Z, p.Wb, p.part, R, l.m, 1, p.ctl, 0);                        // Z^T W and W^T W
    DPB_BY_RANK(l.m, DPB_LAUNCH((fm_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.part, p.S, p.lam, p.A, p.ctl, l.nch, l.m, max_iter));
    DPB_LAUNCH(fm_move_kernel, gc, t256, 0, st, p.Z, p.Wb, p.S, p.A, p.lam, p.Z1, p.respart, R, l.m, p.ctl);    // Z1 = W S V D^-1/2, the residual
    fm_orth_pass(p, l, p.Z1, p.Z, R, r, tol, 1, st);                                                            // Z = Z1 (Z1^T Z1)^-1/2 unless converged
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_mean_finish(const float* X, const double* ghat, long B, int k, long N, int r, long max_iter, float* Y, float* weight, float* theta, double* Ct,
                            double* info, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FmLayout l;
  if (fm_check("dpb_flag_mean_finish", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, l) != 0) return -1;
  const FmPtrs p = fm_ptrs(scratch, l, ghat);
  const int R = (int)(B * k), nb = (int)B;
  const dim3 gc(l.nch), gb((unsigned)B), one(1), t256(256);
  fm_product(p, l, R, 1, st);
  DPB_LAUNCH(fm_gram_kernel, gc, t256, 0, st, p.Z, p.Wb, p.part, R, l.m, 1, p.ctl, 1);
  DPB_BY_RANK(l.m, DPB_LAUNCH((fm_finish_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.part, p.G, p.S, weight, info, p.ctl, l.nch, l.m, r, nb, k, (long)R));
  DPB_LAUNCH(fm_rowmul_kernel, gc, t256, 0, st, p.Z, p.S, Ct, R, l.m, r, p.ctl, 1);                  // C^T = Z Sc
  DPB_LAUNCH(fm_rowmul_kernel, gc, t256, 0, st, p.Wb, p.S, p.Z1, R, l.m, r, p.ctl, 1);               // M^T = Ghat C^T
  DPB_LAUNCH(fm_sign_kernel, one, t256, 0, st, Ct, p.sgn, (long)R, r);
  DPB_LAUNCH(fm_coef_kernel, gb, t256, 0, st, Ct, p.Z1, p.sgn, X ? p.W : nullptr, p.G, p.Wb, k, r, (long)R);
  { const int kr = k > r ? k : r; DPB_BY_RANK(kr, DPB_LAUNCH((fm_theta_kernel<KM, NT>), gb, dim3(NT), 0, st, p.Z1, theta, k, r)); }
  if (X && launch_coef_stream(X, p.Wb, Y, R, r, N, st) != 0) return -1;
  DPB_CHECK(hipGetLastError());
  return 0;
}

// ============================================================================================================ the weighted mean and the flag median
// Weighted flag mean: P_w = (1/B) sum_i what_i Q_i^T Q_i, what of mean 1.  With D = diag(sqrt(what_i) (x) 1_k) the rows D Q have the Gram D Ghat D, so the
// solver above runs unchanged on W = D Ghat D Z -- the scale meets the Z operand before its MFMAs and the output row as it is stored; no scaled copy of Ghat
// exists -- and Y = C~ D Q: the coefficients on Q are C^T = D C~^T, C Ghat C^T = I.  The affinities of ALL members (weight 0 included) come from the
// unweighted product M^T = Ghat C^T: a_i = ||M[i-rows]||_F^2.
// Flag median (Mankovich et al., CVPR 2022): argmin_Y sum_i p_i d_i, d_i = sqrt(r - a_i), by iteratively reweighted flag means, w_i = p_i / max(d_i, eps)
// normalised to mean 1; a round = the inner solve (warm-started: the block Z stays), the Rayleigh-Ritz step of finish, M, a, d, the smoothed objective
// J = sum_i p_i phi(d_i) (phi(d) = d above eps, d^2 / (2 eps) + eps / 2 below: what the clamped weight descends) and the new table.
struct FmedHead {         // the first 64 bytes of a median scratch block (documented in dpb.h: the caller's one read per round or chunk)
  int round;              // objective evaluations so far
  int done, iters;        // the inner solve's status (FmCtl), as of the last call
  int n_degenerate;
  int converged;          // J_prev - J <= tol J_prev was met: the table was not moved
  int pad;
  double J, Jprev, res;
  double pad1, pad2;
};
static_assert(sizeof(FmedHead) == 64, "FmedHead is documented as 64 bytes");

// fm_load's operands and the four table entries sw [R] = sqrt(what_{row / k}) of the lane's rows of Z, read through L2 beside them.  The loads stay as
// fm_load issues them -- nothing waits on them where they are issued -- and the scale meets the Z operand in fmw_mma, just before the MFMAs that use it
template <int KT>
struct FmwOperands {
  double a[2][4];
  double b[4][KT];
  double s[4];
};

template <int KT>
__device__ __forceinline__ void fmw_load(FmwOperands<KT>& o, const double* __restrict__ G, const double* __restrict__ Z, const double* __restrict__ sw, int c,
                                         int c_hi, int i0, int j, int g, int R, int m, bool vec) {
  const int col = 16 * c + 4 * g;
  const bool live = c < c_hi;
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const int row = i0 + 16 * tl + j;
    const bool ok = live && row < R && col < R;
    if (ok && vec) {
      const geom_d4 v = *reinterpret_cast<const geom_d4*>(G + (long)row * R + col);
      o.a[tl][0] = v[0]; o.a[tl][1] = v[1]; o.a[tl][2] = v[2]; o.a[tl][3] = v[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o.a[tl][e] = (ok && col + e < R) ? G[(long)row * R + col + e] : 0.0;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int zr = col + e;
    o.s[e] = (live && zr < R) ? sw[zr] : 0.0;
#pragma unroll
    for (int n = 0; n < KT; ++n) o.b[e][n] = (live && zr < R && 16 * n + j < m) ? Z[(long)zr * m + 16 * n + j] : 0.0;
  }
}

template <int KT>
__device__ __forceinline__ void fmw_mma(geom_d4 (&acc)[2][KT], const FmwOperands<KT>& o) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int n = 0; n < KT; ++n) {
      const double b = o.b[e][n] * o.s[e];
      acc[0][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[0][e], b, acc[0][n], 0, 0, 0);
      acc[1][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[1][e], b, acc[1][n], 0, 0, 0);
    }
}

// Out = D Ghat D Z: fm_product_kernel's pass, cut points and wave-order sum, with the two scales (sw all ones: its bits)
template <int KT, int NW>
__global__ __launch_bounds__(NW * 64) void fmw_product_kernel(const double* __restrict__ G, const double* __restrict__ Z, const double* __restrict__ sw,
                                                              double* __restrict__ Out, int R, int m, const FmCtl* ctl, int force) {
  if (!force && ctl->done) return;
  __shared__ double red[NW][2][KT][4][64];
  static_assert(sizeof(double) * NW * 2 * KT * 4 * 64 <= 160 * 1024, "fmw_product_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * 32;
  const int chunks = (R + 15) / 16, q = (chunks + NW - 1) / NW;
  const int c_lo = wave * q, c_hi = c_lo + q < chunks ? c_lo + q : chunks;
  const bool vec = (R & 3) == 0;
  geom_d4 acc[2][KT];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int n = 0; n < KT; ++n) acc[tl][n] = geom_d4{0.0, 0.0, 0.0, 0.0};
  FmwOperands<KT> o0, o1;
  fmw_load<KT>(o0, G, Z, sw, c_lo, c_hi, i0, j, g, R, m, vec);
  for (int c = c_lo; c < c_hi; c += 2) {
    fmw_load<KT>(o1, G, Z, sw, c + 1, c_hi, i0, j, g, R, m, vec);
    fmw_mma<KT>(acc, o0);
    fmw_load<KT>(o0, G, Z, sw, c + 2, c_hi, i0, j, g, R, m, vec);
    fmw_mma<KT>(acc, o1);
  }
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int n = 0; n < KT; ++n)
#pragma unroll
      for (int x = 0; x < 4; ++x) red[wave][tl][n][x][lane] = acc[tl][n][x];
  __syncthreads();
  for (int e = t; e < 2 * KT * 4 * 64; e += NW * 64) {
    const int ln = e & 63, x = (e >> 6) & 3, n = (e >> 8) % KT, tl = (e >> 8) / KT;
    double v = red[0][tl][n][x][ln];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w][tl][n][x][ln];
    const int row = i0 + 16 * tl + (ln >> 4) + 4 * x, col = 16 * n + (ln & 15);
    if (row < R && col < m) Out[(long)row * m + col] = v * sw[row];
  }
}

// one workgroup: the prior p (given weights w [B] scaled to mean 1, the sum in index order; w == nullptr: all ones), what = p, the table and the head.
// A negative or non-finite weight, or a zero sum, gives a NaN table: the solver then ends with the degenerate status
__global__ __launch_bounds__(256) void fmed_init_kernel(const double* w, const double* G, double* prior, double* what, double* sw, FmedHead* head, int B, int k,
                                                        long R) {
  __shared__ double tot;
  __shared__ int nd;
  const int t = threadIdx.x;
  if (t == 0) {
    double s = 0.0;
    int n = 0;
    for (int i = 0; i < B; ++i) {
      s += w ? w[i] : 1.0;
      const double d = G[((long)i * k) * (R + 1)];
      if (d != d) n += 1;
    }
    tot = s; nd = n;
  }
  __syncthreads();
  for (int i = t; i < B; i += 256) {
    const double wi = w ? w[i] : 1.0;
    const double p = w ? ((wi >= 0.0 && tot > 0.0) ? wi * (double)B / tot : nan64()) : 1.0;
    prior[i] = p; what[i] = p;
  }
  for (long e = t; e < R; e += 256) {
    const double wi = w ? w[e / k] : 1.0;
    const double p = w ? ((wi >= 0.0 && tot > 0.0) ? wi * (double)B / tot : nan64()) : 1.0;
    sw[e] = sqrt(p);
  }
  if (t == 0) {
    head->round = 0; head->done = 0; head->iters = 0; head->n_degenerate = nd; head->converged = 0; head->pad = 0;
    head->J = 0.0; head->Jprev = 0.0; head->res = 0.0; head->pad1 = 0.0; head->pad2 = 0.0;
  }
}

// the inner solve's status copied to the head (the caller's read)
__global__ void fmed_sync_kernel(const FmCtl* ctl, FmedHead* head) {
  head->done = ctl->done; head->iters = ctl->iters; head->res = ctl->res;
}

// Ct [R][r] rows scaled by the table: C^T = D C~^T
__global__ __launch_bounds__(256) void fmed_scale_kernel(double* Ct, const double* sw, long R, int r) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < R * r) Ct[e] *= sw[e / r];
}

// block i (one wave): a_i = ||M[i-rows]||_F^2 -- lane-strided squares in element order, then the xor butterfly -- and d_i = sqrt(max(r - a_i, 0))
__global__ __launch_bounds__(64) void fmed_affinity_kernel(const double* Mt, double* aff, double* dist, int k, int r) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const double* Mb = Mt + (long)i * k * r;
  double sq = 0.0;
  for (int e = lane; e < k * r; e += 64) { const double v = Mb[e]; sq += v * v; }
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if (lane == 0) {
    const double x = (double)r - sq;
    aff[i] = sq;
    dist[i] = x != x ? nan64() : (x > 0.0 ? sqrt(x) : 0.0);
  }
}

// one workgroup, the step of a round: J = sum_i p_i phi_eps(d_i) in index order; converged when round >= 1 and J_prev - J <= tol J_prev; otherwise, with
// update, the new table what_i = w_i B / sum w, w_i = p_i / max(d_i, eps) (the sum in index order), and the inner solve's status cleared -- the block stays
__global__ __launch_bounds__(256) void fmed_step_kernel(const double* prior, const double* dist, double* what, double* sw, FmedHead* head, FmCtl* ctl, int B, int k,
                                                        long R, double eps, double tol, int update) {
  __shared__ double tot;
  __shared__ int move;
  const int t = threadIdx.x;
  if (t == 0) {
    double J = 0.0, s = 0.0;
    for (int i = 0; i < B; ++i) {
      const double d = dist[i], p = prior[i];
      J += p * (d >= eps ? d : d * d / (2.0 * eps) + 0.5 * eps);          // (a NaN distance: the else branch, a NaN)
      s += p / (d > eps ? d : eps);
    }
    const double Jp = head->J;
    const int conv = head->round >= 1 && (Jp - J <= tol * Jp) ? 1 : 0;
    head->Jprev = head->round >= 1 ? Jp : J;
    head->J = J;
    head->round += 1;
    head->converged = conv;
    head->done = ctl->done; head->iters = ctl->iters; head->res = ctl->res;
    move = (update && !conv && J == J && ctl->done != 2) ? 1 : 0;
    tot = s;
  }
  __syncthreads();
  if (!move) return;
  for (int i = t; i < B; i += 256) { const double d = dist[i]; what[i] = prior[i] / (d > eps ? d : eps) * (double)B / tot; }
  for (long e = t; e < R; e += 256) { const double d = dist[e / k]; sw[e] = sqrt(prior[e / k] / (d > eps ? d : eps) * (double)B / tot); }
  if (t == 0) { ctl->done = 0; ctl->iters = 0; ctl->res = 0.0; }
}

// member [3][B] = affinity, distance, member weight
__global__ __launch_bounds__(256) void fmed_member_kernel(const double* aff, const double* dist, const double* what, double* member, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) { member[i] = aff[i]; member[B + i] = dist[i]; member[2 * (long)B + i] = what[i]; }
}

namespace {
struct FmedLayout {
  size_t head = 0, prior = 0, what = 0, aff = 0, dist = 0, sw = 0, wtmp = 0, itmp = 0, fm = 0, total = 0;
  FmLayout l;
};
bool fmed_layout(long B, int k, long N, int r, long max_iter, bool own, FmedLayout& ml) {
  if (!fm_layout(B, k, N, r, max_iter, own, ml.l)) return false;
  ScratchCarver s;
  const size_t bd = (size_t)B * sizeof(double);
  ml.head = s.take(sizeof(FmedHead));
  ml.prior = s.take(bd); ml.what = s.take(bd); ml.aff = s.take(bd); ml.dist = s.take(bd);
  ml.sw = s.take((size_t)B * k * sizeof(double));
  ml.wtmp = s.take(64 * sizeof(float));
  ml.itmp = s.take((72 + (size_t)B) * sizeof(double));
  ml.fm = s.off;
  ml.total = s.off + ml.l.total;
  return true;
}
struct FmedPtrs {
  FmedHead* head; double *prior, *what, *aff, *dist, *sw, *itmp; float* wtmp;
  FmPtrs p;
};
FmedPtrs fmed_ptrs(void* scratch, const FmedLayout& ml, const double* ghat) {
  char* b = (char*)scratch;
  FmedPtrs q;
  q.head = (FmedHead*)(b + ml.head); q.prior = (double*)(b + ml.prior); q.what = (double*)(b + ml.what); q.aff = (double*)(b + ml.aff);
  q.dist = (double*)(b + ml.dist); q.sw = (double*)(b + ml.sw); q.wtmp = (float*)(b + ml.wtmp); q.itmp = (double*)(b + ml.itmp);
  q.p = fm_ptrs(b + ml.fm, ml.l, ghat);
  return q;
}
int fmed_check(const char* who, long B, int k, long N, int r, long max_iter, const double* ghat, const void* scratch, size_t scratch_bytes, FmedLayout& ml) {
  if (!fmed_layout(B, k, N, r, max_iter, ghat == nullptr, ml)) {
    set_error("%s: B=%ld outside [1,65535], k=%d outside [1,%d], N=%ld < k, B k above 2^20, r=%d outside [1,min(%d,B k,N)] or max_iter=%ld outside [0,2^24]",
              who, B, k, FRECHET_MAX_RANK, N, r, FLAG_MEAN_MAX_RANK, max_iter);
    return -1;
  }
  if (ghat && (uintptr_t)ghat % 32) { set_error("%s: Ghat must be 32-byte aligned", who); return -1; }
  return ghat ? check_scratch(who, scratch, scratch_bytes, ml.total, "dpb_flag_median_solver_bytes(%ld, %d, %d, %ld)", B, k, r, max_iter)
              : check_scratch(who, scratch, scratch_bytes, ml.total, "dpb_flag_median_scratch_bytes(%ld, %d, %ld, %d, %ld)", B, k, N, r, max_iter);
}

void fmw_product(const FmedPtrs& q, const FmLayout& l, int R, int force, hipStream_t st) {
  const dim3 grid((R + 31) / 32);
  const FmPtrs& p = q.p;
  if (g_fm_waves == 4) DPB_BY_TILES(l.m, DPB_LAUNCH((fmw_product_kernel<KT, 4>), grid, dim3(256), 0, st, p.G, p.Z, q.sw, p.Wb, R, l.m, p.ctl, force));
  else DPB_BY_TILES(l.m, DPB_LAUNCH((fmw_product_kernel<KT, 8>), grid, dim3(512), 0, st, p.G, p.Z, q.sw, p.Wb, R, l.m, p.ctl, force));
}

// the Rayleigh-Ritz step of the block as it stands under the weighted projector (fm_finish_head_kernel on W = D Ghat D Z), C^T = D Z Sc into Ct [R][r],
// M^T = Ghat C^T (the UNWEIGHTED product: a member of weight 0 keeps its affinity and angles) into Z1, then a and d of every member
void fmed_ritz(const FmedPtrs& q, const FmLayout& l, int R, int r, int B, int k, double* Ct, float* weight, double* info, hipStream_t st) {
  const FmPtrs& p = q.p;
  const dim3 gc(l.nch), one(1), t256(256), grid((R + 31) / 32);
  fmw_product(q, l, R, 1, st);
  DPB_LAUNCH(fm_gram_kernel, gc, t256, 0, st, p.Z, p.Wb, p.part, R, l.m, 1, p.ctl, 1);
  DPB_BY_RANK(l.m, DPB_LAUNCH((fm_finish_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.part, p.G, p.S, weight, info, p.ctl, l.nch, l.m, r, B, k, (long)R));
  DPB_LAUNCH(fm_rowmul_kernel, gc, t256, 0, st, p.Z, p.S, Ct, R, l.m, r, p.ctl, 1);
  DPB_LAUNCH(fmed_scale_kernel, dim3((unsigned)(((long)R * r + 255) / 256)), t256, 0, st, Ct, q.sw, (long)R, r);
  if (g_fm_waves == 4) DPB_BY_TILES(r, DPB_LAUNCH((fm_product_kernel<KT, 4>), grid, dim3(256), 0, st, p.G, Ct, p.Z1, R, r, p.ctl, 1));
  else DPB_BY_TILES(r, DPB_LAUNCH((fm_product_kernel<KT, 8>), grid, dim3(512), 0, st, p.G, Ct, p.Z1, R, r, p.ctl, 1));
  DPB_LAUNCH(fmed_affinity_kernel, dim3((unsigned)B), dim3(64), 0, st, p.Z1, q.aff, q.dist, k, r);
}
}  // namespace

size_t flag_median_scratch_bytes(long B, int k, long N, int r, long max_iter, bool own) {
  FmedLayout ml;
  return fmed_layout(B, k, N, r, max_iter, own, ml) ? ml.total : 0;
}

int launch_flag_median_init(const float* X, const double* ghat, const double* member_weight, long B, int k, long N, int r, unsigned long long seed, long max_iter,
                            void* scratch, size_t scratch_bytes, hipStream_t st) {
  FmedLayout ml;
  if (fmed_check("dpb_flag_median_init", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, ml) != 0) return -1;
  const FmedPtrs q = fmed_ptrs(scratch, ml, ghat);
  // the flag mean's own init on the embedded block: Ghat (or the caller's), the start block, the status
  if (launch_flag_mean_init(X, ghat, B, k, N, r, seed, max_iter, (char*)scratch + ml.fm, ml.l.total, st) != 0) return -1;
  DPB_LAUNCH(fmed_init_kernel, dim3(1), dim3(256), 0, st, member_weight, q.p.G, q.prior, q.what, q.sw, q.head, (int)B, k, (long)(B * k));
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_median_iterate(const double* ghat, long B, int k, long N, int r, long max_iter, int n_iter, double tol, void* scratch, size_t scratch_bytes,
                               hipStream_t st) {
  FmedLayout ml;
  if (fmed_check("dpb_flag_median_iterate", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, ml) != 0) return -1;
  if (n_iter < 0 || !(tol >= 0.0)) { set_error("dpb_flag_median_iterate: n_iter=%d < 0 or tol=%g < 0", n_iter, tol); return -1; }
  const FmedPtrs q = fmed_ptrs(scratch, ml, ghat);
  const FmPtrs& p = q.p;
  const FmLayout& l = ml.l;
  const int R = (int)(B * k);
  const dim3 gc(l.nch), one(1), t256(256);
  for (int it = 0; it < n_iter; ++it) {                   // launch_flag_mean_iterate's iteration with the weighted product
    fmw_product(q, l, R, 0, st);
    DPB_LAUNCH(fm_gram_kernel, gc, t256, 0, st, p.Z, p.Wb, p.part, R, l.m, 1, p.ctl, 0);
    DPB_BY_RANK(l.m, DPB_LAUNCH((fm_head_kernel<KM, NT>), one, dim3(NT), 0, st, p.part, p.S, p.lam, p.A, p.ctl, l.nch, l.m, max_iter));
    DPB_LAUNCH(fm_move_kernel, gc, t256, 0, st, p.Z, p.Wb, p.S, p.A, p.lam, p.Z1, p.respart, R, l.m, p.ctl);
    fm_orth_pass(p, l, p.Z1, p.Z, R, r, tol, 1, st);
  }
  DPB_LAUNCH(fmed_sync_kernel, one, one, 0, st, p.ctl, q.head);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_median_round(const double* ghat, long B, int k, long N, int r, long max_iter, double eps, double tol, int update, void* scratch,
                             size_t scratch_bytes, hipStream_t st) {
  FmedLayout ml;
  if (fmed_check("dpb_flag_median_round", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, ml) != 0) return -1;
  if (r > k) { set_error("dpb_flag_median_round: r=%d outside [1,k=%d]: the distance sqrt(r - a) is defined for r <= k only", r, k); return -1; }
  if (!(eps > 0.0) || !(tol >= 0.0)) { set_error("dpb_flag_median_round: eps=%g <= 0 or tol=%g < 0", eps, tol); return -1; }
  const FmedPtrs q = fmed_ptrs(scratch, ml, ghat);
  const int R = (int)(B * k);
  fmed_ritz(q, ml.l, R, r, (int)B, k, q.p.Wb, q.wtmp, q.itmp, st);       // (Wb is free once the head has run: the coefficients take it)
  DPB_LAUNCH(fmed_step_kernel, dim3(1), dim3(256), 0, st, q.prior, q.dist, q.what, q.sw, q.head, q.p.ctl, (int)B, k, (long)R, eps, tol, update ? 1 : 0);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_median_finish(const float* X, const double* ghat, long B, int k, long N, int r, long max_iter, float* Y, float* weight, float* theta, double* Ct,
                              double* member, double* info, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FmedLayout ml;
  if (fmed_check("dpb_flag_median_finish", B, k, N, r, max_iter, ghat, scratch, scratch_bytes, ml) != 0) return -1;
  const FmedPtrs q = fmed_ptrs(scratch, ml, ghat);
  const FmPtrs& p = q.p;
  const int R = (int)(B * k), nb = (int)B;
  const dim3 gb((unsigned)B), one(1), t256(256);
  fmed_ritz(q, ml.l, R, r, nb, k, Ct, weight, info, st);
  DPB_LAUNCH(fmed_member_kernel, dim3((unsigned)((B + 255) / 256)), t256, 0, st, q.aff, q.dist, q.what, member, nb);
  DPB_LAUNCH(fm_sign_kernel, one, t256, 0, st, Ct, p.sgn, (long)R, r);
  DPB_LAUNCH(fm_coef_kernel, gb, t256, 0, st, Ct, p.Z1, p.sgn, X ? p.W : nullptr, p.G, p.Wb, k, r, (long)R);
  { const int kr = k > r ? k : r; DPB_BY_RANK(kr, DPB_LAUNCH((fm_theta_kernel<KM, NT>), gb, dim3(NT), 0, st, p.Z1, theta, k, r)); }
  if (X && launch_coef_stream(X, p.Wb, Y, R, r, N, st) != 0) return -1;
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
